// Life cycle of an engine: umgen_create -- config checks, the two decode engines' censuses, the overlap decision with its streams, the
// state-dict table, workspaces, caches and engine buffers, as stages in that order -- and umgen_destroy; the device allocator and the slot caches.
#include "engine_state.h"

// host arithmetic stays unfused in every engine file, as it was while they were one file behind the numpy-faithful helpers (engine_weights.hip)
#pragma clang fp contract(off)

namespace {

void reg(umgen_engine* e, const std::string& key, void* dst, std::vector<int64_t> shape, int kind, bool optional = false) {
    e->slots[key] = Slot{dst, std::move(shape), kind, false, optional};
}

int alloc_f32(umgen_engine* e, const std::string& key, float** p, std::vector<int64_t> shape) {
    size_t n = 1;
    for (auto d : shape) n *= (size_t)d;
    if (int rc = dalloc(e, p, n)) return rc;
    reg(e, key, *p, shape, 0);
    return 0;
}
int alloc_w(umgen_engine* e, const std::string& key, void** p, std::vector<int64_t> shape) {
    size_t n = 1;
    for (auto d : shape) n *= (size_t)d;
    if (int rc = dev_alloc(e, p, n * e->tsz)) return rc;
    reg(e, key, *p, shape, 1);
    return 0;
}

int alloc_attn(umgen_engine* e, const std::string& pre, AttnW& a) {
    const int64_t E = e->E;
    if (int rc = alloc_w(e, pre + ".c_attn.weight", &a.Wqkv, {3 * E, E})) return rc;
    if (int rc = alloc_f32(e, pre + ".c_attn.bias", &a.bqkv, {3 * E})) return rc;
    if (int rc = alloc_w(e, pre + ".c_proj.weight", &a.Wo, {E, E})) return rc;
    return alloc_f32(e, pre + ".c_proj.bias", &a.bo, {E});
}
int alloc_mlp(umgen_engine* e, const std::string& pre, MlpW& m) {
    const int64_t E = e->E;
    if (int rc = alloc_w(e, pre + ".c_fc.weight", &m.Wfc, {4 * E, E})) return rc;
    return alloc_w(e, pre + ".c_proj.weight", &m.Wproj, {E, 4 * E});
}
int alloc_sub(umgen_engine* e, const std::string& pre, const char* ln_a, const char* attn, const char* ln_b, const char* mlp, SubW& s) {
    const int64_t E = e->E;
    if (int rc = alloc_f32(e, pre + "." + ln_a + ".weight", &s.ln_a, {E})) return rc;
    if (int rc = alloc_attn(e, pre + "." + attn, s.attn)) return rc;
    if (int rc = alloc_f32(e, pre + "." + ln_b + ".weight", &s.ln_b, {E})) return rc;
    return alloc_mlp(e, pre + "." + mlp, s.mlp);
}

}  // namespace

namespace umgen {

int dev_alloc(umgen_engine* e, void** p, size_t bytes) {
    HIPCHK(e, hipMalloc(p, bytes ? bytes : 16));
    e->allocs.push_back(*p);
    return 0;
}

// Slot caches of the temporal sub-blocks: per stack and block [max_batch][max_cond_frames][S_stack][2E] of T (10.5 GB per scene for
// UMGen_Large in 16 bits -- what the 288 GB are for).  Allocated once, at create for the overlapped pass or on the first frame whose
// window will grow; when they would take more than half of the free memory the engine keeps recomputing the window (tcache_state -1).
bool ensure_tcache(umgen_engine* e) {
    if (e->tcache_state) return e->tcache_state > 0;
    const size_t Bm = e->cfg.max_batch, Tm = e->cfg.max_cond_frames;
    size_t free_b = 0, total_b = 0, need = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); e->tcache_state = -1; return false; }
    for (int st = 0; st < 4; ++st) need += e->stk[st].size() * Bm * Tm * (size_t)stack_len(st) * 2 * e->E * e->tsz;
    if (need > free_b / 2) { e->tcache_state = -1; return false; }
    for (int st = 0; st < 4; ++st) {
        e->tcache[st].assign(e->stk[st].size(), nullptr);
        for (auto& c : e->tcache[st])
            if (dev_alloc(e, &c, Bm * Tm * (size_t)stack_len(st) * 2 * e->E * e->tsz)) {
                // partial failure: the caches allocated so far would stay reserved and unused for the engine's life -- give them back
                (void)hipGetLastError();
                for (int s2 = 0; s2 <= st; ++s2) {
                    for (void*& p : e->tcache[s2])
                        if (p) {
                            e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), p), e->allocs.end());
                            (void)hipFree(p);
                            p = nullptr;
                        }
                    e->tcache[s2].clear();
                }
                e->tcache_state = -1;
                return false;
            }
    }
    e->tcache_state = 1;
    return true;
}

}  // namespace umgen

namespace {

// what the stages of umgen_create share beside the engine: the caller's config and the two switches that more than one decision reads
struct CreateCtx {
    const umgen_config* cfg;
    const char *de_env, *ov_env;      // UMGEN_DECODE_ENGINE, UMGEN_OVERLAP
};

int validate_config(umgen_engine* e, const umgen_config* cfg) {
    if (cfg->abi_version != UMGEN_ABI_VERSION) return e->fail(UMGEN_E_INVALID, "abi_version %d != %d", cfg->abi_version, UMGEN_ABI_VERSION);
    if (cfg->n_head <= 0 || cfg->n_embd != cfg->n_head * kHeadDim)
        return e->fail(UMGEN_E_UNSUPPORTED, "head_dim must be %d (n_embd=%d, n_head=%d)", kHeadDim, cfg->n_embd, cfg->n_head);
    if (cfg->n_embd > 1536) return e->fail(UMGEN_E_UNSUPPORTED, "n_embd <= 1536 supported");
    if (cfg->map_vocab > 8192 || cfg->img_vocab > 8192 || cfg->bbox3d_vocab != 1028 || cfg->pose_vocab > 8192)
        return e->fail(UMGEN_E_UNSUPPORTED, "vocab sizes out of range");
    if (cfg->max_cond_frames > 64) return e->fail(UMGEN_E_UNSUPPORTED, "max_cond_frames <= 64 supported (temporal attention tile)");
    if (cfg->max_batch < 1 || cfg->max_cond_frames < 1 || cfg->max_cond_frames > cfg->max_frame_len)
        return e->fail(UMGEN_E_INVALID, "max_batch / max_cond_frames invalid");
    if (cfg->precision != UMGEN_PREC_FP32 && cfg->precision != UMGEN_PREC_BF16 && cfg->precision != UMGEN_PREC_FP16)
        return e->fail(UMGEN_E_INVALID, "precision %d (UMGEN_PREC_FP32 / _BF16 / _FP16)", cfg->precision);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return e->fail(UMGEN_E_HIP, "no HIP device visible: libumgen_hip has no CPU fallback");
    HIPCHK(e, hipSetDevice(cfg->device));
    HIPCHK(e, gemm256_prepare());   // per device: dynamic-LDS attribute + CU count of the 256 x 256 GEMM (a second GPU in one process gets its own)
    return 0;
}

int census_xcd_engine(umgen_engine* e, const CreateCtx& cc) {
    const umgen_config* cfg = cc.cfg;
    const char *de_env = cc.de_env, *ov_env = cc.ov_env;
    // hand-off tags: (round or scene, layer, edge) of one step must fit kEpochPerStep (oar_engine.hip): <= 64 layers; up to 32 scenes flow
    // through the systolic schedule, more run as rounds of 8 whole-scene groups (<= 32 rounds)
    const bool engine_wanted = cfg->precision != UMGEN_PREC_FP32 && cfg->n_embd == kEngE && cfg->n_head == kEngH && cfg->n_oar_layer <= 64 &&
                               cfg->max_batch <= 256 && !(de_env && de_env[0] == '0') && !(ov_env && ov_env[0] != '0');
    if (engine_wanted) {
        // Census FIRST, on the plain stream the engine would use: an engine-shaped launch (one 512-thread workgroup per CU) must put
        // exactly 32 workgroups on each of 8 XCDs, twice in a row with the same XCD map.  Only when that holds is the overlap given
        // up for the engine; otherwise (partitioned GPU, another SKU, CUs busy with somebody else's persistent kernel) the engine
        // falls back to the five-launch decode layer WITH the overlapped TAR pass, and says so.
        HIPCHK(e, hipStreamCreate(&e->stream));
        HIPCHK(e, oar_engine_prepare());
        unsigned* d_cnt = nullptr;
        HIPCHK(e, hipMalloc(&d_cnt, 64));
        umgen_engine::EngStream& es = e->eng_fg;
        es.ok = true;
        for (int rep = 0; rep < 2 && es.ok; ++rep) {
            unsigned cnt[16] = {};
            if (hipMemsetAsync(d_cnt, 0, 64, e->stream) != hipSuccess || launch_oar_engine_census(e->stream, 8, d_cnt) != hipSuccess ||
                hipMemcpyAsync(cnt, d_cnt, 64, hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) {
                (void)hipGetLastError();
                es.ok = false;
                break;
            }
            if (getenv("UMGEN_DEBUG_TIMING")) {
                fprintf(stderr, "[umgen] engine census:");
                for (int x = 0; x < 16; ++x) fprintf(stderr, " %u", cnt[x]);
                fprintf(stderr, "\n");
            }
            int groups = 0;
            unsigned char map[16];
            for (int x = 0; x < 16; ++x) {
                map[x] = 0xff;
                if (cnt[x] == (unsigned)kEngGroup) map[x] = (unsigned char)groups++;
                else if (cnt[x] != 0) es.ok = false;
            }
            if (groups != 8 || (rep == 1 && memcmp(map, es.map, 16))) es.ok = false;
            memcpy(es.map, map, 16);
        }
        (void)hipFree(d_cnt);
        es.NG = 8;
        e->eng_enabled = es.ok;
        if (!es.ok) {
            e->eng_fallback = true;
            fprintf(stderr, "[umgen] WARNING: the XCD-resident decode engine cannot be used on device %d (its census did not find 32 workgroups on each "
                            "of 8 XCDs); decode steps run as five launches per layer (~30 %% slower at one scene per GPU)\n", cfg->device);
            HIPCHK(e, hipStreamDestroy(e->stream));
            e->stream = nullptr;
        }
    }
    return 0;
}

int census_wide_engine(umgen_engine* e, const CreateCtx& cc) {
    const umgen_config* cfg = cc.cfg;
    const char* ov_env = cc.ov_env;
    // Wide layers (n_embd 1536): the chip-wide engine needs all 256 CUs of the decode stream at once (one persistent workgroup per CU: the same
    // census as the XCD-resident engine's, 32 workgroups on each of 8 XCDs, twice) and, like it, gives up the CU-masked background TAR pass.
    const char* dw_env = getenv("UMGEN_DECODE_WIDE");
    if (cfg->precision != UMGEN_PREC_FP32 && cfg->n_embd == kWideE && cfg->n_head == kWideE / kHeadDim && cfg->n_oar_layer <= 64 &&
        cfg->max_batch <= std::max(0, std::min(4, dw_env ? atoi(dw_env) : 1)) && !(ov_env && ov_env[0] != '0')) {
        HIPCHK(e, hipStreamCreate(&e->stream));
        HIPCHK(e, oar_engine_wide_prepare());
        unsigned* d_cnt = nullptr;
        HIPCHK(e, hipMalloc(&d_cnt, 64));
        bool ok = true;
        for (int rep2 = 0; rep2 < 2 && ok; ++rep2) {
            unsigned cnt[16] = {};
            if (hipMemsetAsync(d_cnt, 0, 64, e->stream) != hipSuccess || launch_oar_engine_wide_census(e->stream, d_cnt) != hipSuccess ||
                hipMemcpyAsync(cnt, d_cnt, 64, hipMemcpyDeviceToHost, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) {
                (void)hipGetLastError();
                ok = false;
                break;
            }
            int groups = 0;
            for (int x = 0; x < 16; ++x) {
                if (cnt[x] == (unsigned)kEngGroup) ++groups;
                else if (cnt[x] != 0) ok = false;
            }
            if (groups != 8) ok = false;
        }
        (void)hipFree(d_cnt);
        e->wide_enabled = ok;
        if (!ok) {
            fprintf(stderr, "[umgen] WARNING: the chip-wide decode engine cannot be used on device %d (its census did not find one workgroup on each of 256 "
                            "CUs); decode steps run as five launches per layer\n", cfg->device);
            HIPCHK(e, hipStreamDestroy(e->stream));
            e->stream = nullptr;
        }
    }
    return 0;
}

int choose_overlap(umgen_engine* e, const CreateCtx& cc) {
    const umgen_config* cfg = cc.cfg;
    const char* ov_env = cc.ov_env;
    e->overlap = cfg->max_cond_frames >= 2 && !e->eng_enabled && !e->wide_enabled;
    if (ov_env) { e->overlap_mode = ov_env[0] - '0'; e->overlap = cfg->max_cond_frames >= 2 && ov_env[0] != '0'; }
    // One scene per GPU on the XCD-resident engine: the overlapped pass runs on the engine's idle XCDs (bg_worker.h; UMGEN_BG_ENGINE=0: the engine on all
    // eight groups and every frame's whole window in the foreground, as in rounds 2-5).  Engines for more scenes keep every XCD busy with the decode.
    const char* be_env = getenv("UMGEN_BG_ENGINE");
    e->bg_engine = e->eng_enabled && cfg->max_batch == 1 && cfg->max_cond_frames >= 2 && cfg->max_cond_frames <= 32 && !ov_env && !(be_env && be_env[0] == '0');
    if (e->bg_engine) { e->overlap = true; e->overlap_mode = 1; }
    int bg_cus = 64;   // mask bits are striped over the 8 XCDs: 64 = 8 CUs of each XCD for the background stream
    if (const char* bc = getenv("UMGEN_BG_CUS")) bg_cus = std::max(32, std::min(128, atoi(bc)));
    if (e->bg_engine) {
        void* qp = nullptr;
        if (int rc = dev_alloc(e, &qp, sizeof(BgQueue))) return rc;
        e->d_bgq = reinterpret_cast<BgQueue*>(qp);
        HIPCHK(e, hipMemset(e->d_bgq, 0, sizeof(BgQueue)));
        HIPCHK(e, hipEventCreate(&e->ev_drain0));
        HIPCHK(e, hipEventCreate(&e->ev_drain1));
    }
    if (e->overlap && !e->bg_engine) {
        hipDeviceProp_t prop;
        HIPCHK(e, hipGetDeviceProperties(&prop, cfg->device));
        const int ncu = prop.multiProcessorCount;
        if (ncu < 2 * bg_cus) e->overlap = false;
        else {
            std::vector<uint32_t> mbg((ncu + 31) / 32, 0u), mfg((ncu + 31) / 32, 0u);
            int fg_cus = ncu - bg_cus;   // UMGEN_FG_CUS: experiment, decode loop on fewer CUs
            if (const char* fc = getenv("UMGEN_FG_CUS")) fg_cus = std::max(32, std::min(ncu - bg_cus, atoi(fc)));
            e->fg_xcds = fg_cus / 32;
            for (int cu = 0; cu < ncu; ++cu) {
                if (cu < bg_cus) mbg[cu / 32] |= 1u << (cu % 32);
                else if (cu < bg_cus + fg_cus) mfg[cu / 32] |= 1u << (cu % 32);
            }
            // a device that refuses CU masks (e.g. a partitioned GPU) simply runs the plain one-stream path: same HIP kernels, same tokens
            if (hipExtStreamCreateWithCUMask(&e->stream, (uint32_t)mfg.size(), mfg.data()) != hipSuccess ||
                hipExtStreamCreateWithCUMask(&e->bg_stream, (uint32_t)mbg.size(), mbg.data()) != hipSuccess) {
                (void)hipGetLastError();
                if (e->stream) { hipStreamDestroy(e->stream); e->stream = nullptr; }
                if (e->bg_stream) { hipStreamDestroy(e->bg_stream); e->bg_stream = nullptr; }
                e->overlap = false;
            } else {
                HIPCHK(e, hipStreamCreateWithFlags(&e->full_stream, hipStreamNonBlocking));
                HIPCHK(e, hipEventCreate(&e->ev_pre_done));
                HIPCHK(e, hipEventCreate(&e->ev_tar_done));
                HIPCHK(e, hipEventCreate(&e->ev_bg_done));
                HIPCHK(e, hipEventCreate(&e->ev_bg0));
            }
        }
    }
    if (!e->stream) HIPCHK(e, hipStreamCreate(&e->stream));
    for (auto& ev : e->ev) HIPCHK(e, hipEventCreate(&ev));
    return 0;
}

int register_parameters(umgen_engine* e, const umgen_config* cfg) {
    e->E = cfg->n_embd;
    e->H = cfg->n_head;
    if (const char* sl = getenv("UMGEN_DEBUG_SAME_LAYER")) e->dbg_same_layer = sl[0] == '1';
    if (const char* rb = getenv("UMGEN_ROWS_PER_BLOCK")) e->rows_per_block = rb[0] - '0';
    e->tsz = cfg->precision == UMGEN_PREC_FP32 ? 4 : 2;
    const int64_t E = e->E;
    const std::string t = "transformer.";
    // ---- parameters (names = the reference state-dict keys, UMGen.py:176-261) ----
    float* tmp;
    if (int rc = alloc_f32(e, t + "egoe.weight", &tmp, {3, E})) return rc; e->tb.egoe = tmp;
    if (int rc = alloc_f32(e, t + "axe.weight", &tmp, {cfg->aux_vocab, E})) return rc; e->tb.axe = tmp;
    if (int rc = alloc_f32(e, t + "be.weight", &tmp, {cfg->bbox3d_vocab, E})) return rc; e->tb.be = tmp;
    if (int rc = alloc_f32(e, t + "tpe.weight", &tmp, {cfg->max_frame_len, E})) return rc; e->tb.tpe = tmp;
    if (int rc = alloc_f32(e, t + "spe.weight", &tmp, {kSeq, E})) return rc; e->tb.spe = tmp;
    if (int rc = alloc_f32(e, t + "tske.weight", &tmp, {cfg->task_num, E})) return rc; e->tb.tske = tmp;
    e->tb.E = e->E;
    const char* stack_name[4] = {"ego_tar", "map_tar", "box_tar", "TAR"};
    const int stack_n[4] = {cfg->n_ego_tar_layer, cfg->n_map_tar_layer, cfg->n_box_tar_layer, cfg->n_tar_layer};
    for (int s = 0; s < 4; ++s) {
        e->stk[s].resize(stack_n[s]);
        for (int i = 0; i < stack_n[s]; ++i) {
            const std::string pre = t + stack_name[s] + "." + std::to_string(i);
            TarW& b = e->stk[s][i];
            if (int rc = alloc_sub(e, pre, "ln_1", "spatial_attn_1", "ln_2", "mlp1", b.sub[0])) return rc;
            if (int rc = alloc_sub(e, pre, "ln_3", "temporal_attn", "ln_4", "mlp2", b.sub[1])) return rc;
            if (int rc = alloc_sub(e, pre, "ln_5", "spatial_attn_2", "ln_6", "mlp3", b.sub[2])) return rc;
        }
    }
    e->oar.resize(cfg->n_oar_layer);
    for (int i = 0; i < cfg->n_oar_layer; ++i)
        if (int rc = alloc_sub(e, t + "OAR." + std::to_string(i), "ln_1", "temporal_attn", "ln_2", "mlp", e->oar[i])) return rc;
    e->dec.resize(cfg->n_ego_ca_layer);
    for (int i = 0; i < cfg->n_ego_ca_layer; ++i) {
        const std::string pre = t + "ego_cross_attn." + std::to_string(i);
        DecW& d = e->dec[i];
        if (int rc = alloc_f32(e, pre + ".ln_1.weight", &d.ln1, {E})) return rc;
        if (int rc = alloc_attn(e, pre + ".self_attn", d.self)) return rc;
        if (int rc = alloc_f32(e, pre + ".ln_2.weight", &d.ln2, {E})) return rc;
        if (int rc = alloc_f32(e, pre + ".ln_3.weight", &d.ln3, {E})) return rc;
        if (int rc = alloc_w(e, pre + ".cross_attn.q_attn.weight", &d.Wq, {E, E})) return rc;
        if (int rc = alloc_f32(e, pre + ".cross_attn.q_attn.bias", &d.bq, {E})) return rc;
        // k_attn | v_attn packed into one [2E][E] projection
        if (int rc = dev_alloc(e, &d.Wkv, (size_t)2 * E * E * e->tsz)) return rc;
        if (int rc = dalloc(e, &d.bkv, (size_t)2 * E)) return rc;
        reg(e, pre + ".cross_attn.k_attn.weight", d.Wkv, {E, E}, 1);
        reg(e, pre + ".cross_attn.v_attn.weight", reinterpret_cast<char*>(d.Wkv) + (size_t)E * E * e->tsz, {E, E}, 1);
        reg(e, pre + ".cross_attn.k_attn.bias", d.bkv, {E}, 0);
        reg(e, pre + ".cross_attn.v_attn.bias", d.bkv + E, {E}, 0);
        if (int rc = alloc_w(e, pre + ".cross_attn.c_proj.weight", &d.Wco, {E, E})) return rc;
        if (int rc = alloc_f32(e, pre + ".cross_attn.c_proj.bias", &d.bco, {E})) return rc;
        if (int rc = alloc_f32(e, pre + ".ln_4.weight", &d.ln4, {E})) return rc;
        if (int rc = alloc_mlp(e, pre + ".mlp1", d.mlp)) return rc;
    }
    if (int rc = alloc_f32(e, t + "ln_ego_tar.weight", &e->ln_ego_tar, {E})) return rc;
    if (int rc = alloc_f32(e, t + "ln_ego.weight", &e->ln_ego, {E})) return rc;
    if (int rc = alloc_f32(e, t + "ln_tar.weight", &e->ln_tar, {E})) return rc;
    if (int rc = alloc_f32(e, t + "ln_oar.weight", &e->ln_oar, {E})) return rc;
    if (int rc = alloc_f32(e, t + "ln_map_tar.weight", &e->ln_map_tar, {E})) return rc;
    if (int rc = alloc_f32(e, t + "ln_box_tar.weight", &e->ln_box_tar, {E})) return rc;
    if (int rc = alloc_w(e, t + "head_ego.weight", &e->head_ego, {cfg->pose_vocab, E})) return rc;
    if (int rc = alloc_w(e, t + "head_ar_map.weight", &e->head_ar_map, {cfg->map_vocab, E})) return rc;
    if (int rc = alloc_w(e, t + "head_ar_bbox3d.weight", &e->head_ar_box, {cfg->bbox3d_vocab, E})) return rc;
    if (int rc = alloc_w(e, t + "head_tar_bbox3d.weight", &e->head_tar_box, {cfg->bbox3d_vocab, E})) return rc;
    if (int rc = alloc_w(e, t + "head_ar_img.weight", &e->head_ar_img, {cfg->img_vocab, E})) return rc;
    if (int rc = alloc_w(e, "map_mlp_pre.c_fc.weight", &e->map_fc, {4 * E, cfg->n_map_embd})) return rc;
    if (int rc = alloc_w(e, "map_mlp_pre.c_proj.weight", &e->map_proj, {E, 4 * E})) return rc;
    if (int rc = alloc_w(e, "img_mlp_pre.c_fc.weight", &e->img_fc, {4 * E, cfg->n_img_embd})) return rc;
    if (int rc = alloc_w(e, "img_mlp_pre.c_proj.weight", &e->img_proj, {E, 4 * E})) return rc;
    if (int rc = alloc_f32(e, "map_codebook.weight", &e->map_cb, {cfg->map_vocab, cfg->n_map_embd})) return rc;
    if (int rc = alloc_f32(e, "img_codebook.weight", &e->img_cb, {cfg->img_vocab, cfg->n_img_embd})) return rc;
    // bf16 constant tables: computed at finalize unless a checkpoint provides them (UMGen.py:257-261)
    bf16_t *fp, *po, *gp;
    if (int rc = dalloc(e, &fp, (size_t)1024 * E)) return rc;
    if (int rc = dalloc(e, &po, (size_t)1030 * E)) return rc;
    if (int rc = dalloc(e, &gp, (size_t)1024 * E)) return rc;
    e->tb.fouier_pe = fp; e->tb.posi = po; e->tb.grid_posi = gp;
    reg(e, "fouier_pe", fp, {1024, E}, 2, true);
    reg(e, "bbox3d_spatial_posi", po, {1030, E}, 2, true);
    reg(e, "grid_center_posi_embedding", gp, {1024, E}, 2, true);
    return 0;
}

int alloc_workspace(umgen_engine* e, const umgen_config* cfg) {
    const int64_t E = e->E;
    // ---- workspace ----
    const size_t Bm = cfg->max_batch, Tm = cfg->max_cond_frames;
    const size_t R = Bm * Tm * kSeq;
    e->S_pad = ((kSeq + 63) / 64) * 64;
    umgen_engine::Work& wm = e->w_main;
    if (int rc = dalloc(e, &wm.X, R * E)) return rc;
    if (int rc = dev_alloc(e, &wm.A, R * E * e->tsz)) return rc;
    if (int rc = dev_alloc(e, &wm.QKV, R * 3 * E * e->tsz)) return rc;
    if (int rc = dev_alloc(e, &wm.VT, Bm * Tm * E * e->S_pad * e->tsz)) return rc;
    HIPCHK(e, hipMemset(wm.VT, 0, Bm * Tm * E * e->S_pad * e->tsz));   // pad columns stay zero forever
    if (int rc = dev_alloc(e, &wm.Hb, R * 4 * E * e->tsz)) return rc;
    if (int rc = dalloc(e, &wm.mapfeat, Bm * Tm * kNMap * E)) return rc;
    if (int rc = dalloc(e, &e->score_part, Bm * kNMap * 8 * 4)) return rc;      // (head_nll_nsplit <= 8)
    if (int rc = dalloc(e, &e->score_logp, Bm * kTokPerFrame)) return rc;
    if (int rc = dalloc(e, &e->score_arg, Bm * kTokPerFrame)) return rc;
    // The three TAR stacks of a frame are independent (UMGen.py:1484-1494 feeds each the same window): in the plain path the map and box
    // stacks run on two side streams with whole-window workspaces of their own, so that the tail of every launch (a persistent GEMM's
    // last partial round of tiles, the ragged last attention blocks, the gaps between dependent launches) is filled by the other
    // stacks' workgroups instead of idling.  (The overlapped pass of round 1 uses the same streams with 1-slot workspaces.)
    const char* cs_env = getenv("UMGEN_CONCURRENT_STACKS");
    e->conc_stacks = !e->overlap && (cs_env ? cs_env[0] != '0' : true);
    if (e->overlap || e->conc_stacks) {   // 1-slot (overlap) / whole-window (concurrent stacks) workspaces + streams
        const size_t slots = e->overlap ? 1 : Tm;
        // the side workspaces hold the map stack (1031 rows per frame) and the box stack (1693), not 2207; when they do not fit beside
        // the main workspace and the caches (a large max_batch), the stacks simply run one behind the other on one stream
        const int side_len[2] = {stack_len(STACK_MAP), stack_len(STACK_BOX)};
        size_t need = 0, free_b = 0, total_b = 0;
        for (int i = 0; i < 2; ++i)
            need += Bm * slots * ((size_t)side_len[i] * E * (4 + 8 * e->tsz) + (size_t)E * e->S_pad * e->tsz + (size_t)kNMap * E * 4);
        HIPCHK(e, hipMemGetInfo(&free_b, &total_b));
        const size_t kv_need = (size_t)cfg->n_oar_layer * Bm * (size_t)e->Lmax * 2 * E * e->tsz;
        if (!e->overlap && need + kv_need > free_b - free_b / 8) {
            e->conc_stacks = false;
            fprintf(stderr, "[umgen] note: %.1f GB of side workspaces for the concurrent map / box stacks do not fit (%.1f GB free): the three TAR stacks run "
                            "one behind the other\n", (double)need / 1e9, (double)free_b / 1e9);
        }
    }
    if (e->overlap || e->conc_stacks) {
        const size_t slots = e->overlap ? 1 : Tm;
        const int side_len[2] = {stack_len(STACK_MAP), stack_len(STACK_BOX)};
        for (int i = 0; i < 2; ++i) {
            const size_t R1 = Bm * slots * (size_t)(e->overlap ? kSeq : side_len[i]);
            umgen_engine::Work& w = e->w_side[i];
            if (int rc = dalloc(e, &w.X, R1 * E)) return rc;
            if (int rc = dev_alloc(e, &w.A, R1 * E * e->tsz)) return rc;
            if (int rc = dev_alloc(e, &w.QKV, R1 * 3 * E * e->tsz)) return rc;
            if (int rc = dev_alloc(e, &w.VT, Bm * slots * E * e->S_pad * e->tsz)) return rc;
            HIPCHK(e, hipMemset(w.VT, 0, Bm * slots * E * e->S_pad * e->tsz));
            if (int rc = dev_alloc(e, &w.Hb, R1 * 4 * E * e->tsz)) return rc;
            if (int rc = dalloc(e, &w.mapfeat, Bm * slots * kNMap * E)) return rc;
            HIPCHK(e, hipStreamCreateWithFlags(&e->side_stream[i], hipStreamNonBlocking));
            HIPCHK(e, hipEventCreate(&e->ev_side_done[i]));
        }
        HIPCHK(e, hipEventCreate(&e->ev_side_in));
    }
    if (int rc = dalloc(e, &e->warped_last, Bm * kNMap * E)) return rc;
    if (int rc = dalloc(e, &e->dv.cond, Bm * kSeq * E)) return rc;
    if (int rc = dalloc(e, &e->pego, Bm * kSeq * E)) return rc;
    if (int rc = dalloc(e, &e->pose_diff, Bm * Tm * 3)) return rc;
    if (int rc = dalloc(e, &e->dv.xdec, 3 * Bm * E)) return rc;
    if (int rc = dalloc(e, &e->dv.qdec, 3 * Bm * E)) return rc;
    if (int rc = dalloc(e, &e->qkv3, 3 * Bm * 3 * E)) return rc;
    if (int rc = dalloc(e, &e->part, 3 * Bm * e->H * kAttnRec)) return rc;
    HIPCHK(e, hipMemset(e->part, 0, 3 * Bm * e->H * kAttnRec * sizeof(float)));   // never-written split slots are read with weight 0
    if (int rc = dalloc(e, &e->hdec, 3 * Bm * 4 * E)) return rc;
    if (int rc = dalloc(e, &e->dv.xfrag, (size_t)kRowsMaxM * E)) return rc;
    if (int rc = dalloc(e, &e->dv.afrag, (size_t)kRowsMaxM * E)) return rc;
    if (int rc = dalloc(e, &e->dv.hfrag, (size_t)kRowsMaxM * 4 * E)) return rc;
    HIPCHK(e, hipMemset(e->dv.xfrag, 0, (size_t)kRowsMaxM * E * 4));       // (columns past the batch are computed, never stored: keep them finite)
    HIPCHK(e, hipMemset(e->dv.afrag, 0, (size_t)kRowsMaxM * E * 4));
    HIPCHK(e, hipMemset(e->dv.hfrag, 0, (size_t)kRowsMaxM * 4 * E * 4));
    return 0;
}

int alloc_decode_buffers(umgen_engine* e, const umgen_config* cfg) {
    const int64_t E = e->E;
    const size_t Bm = cfg->max_batch, Tm = cfg->max_cond_frames;
    if (const char* bd = getenv("UMGEN_DECODE_BATCHED")) e->batched_min = atoi(bd);
    if (const char* dl = getenv("UMGEN_DECODE_LANES")) e->lanes_env = atoi(dl);
    if (e->tsz == 2 && Bm >= 2 && e->lanes_env != 1) {      // decode lanes: streams, step states and fragment buffers (1.2 MB per lane)
        for (auto& ln : e->lane) {
            HIPCHK(e, hipStreamCreateWithFlags(&ln.s, hipStreamNonBlocking));
            HIPCHK(e, hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
            if (int rc = dalloc(e, &ln.st, (size_t)1)) return rc;
            if (int rc = dalloc(e, &ln.xfrag, (size_t)kRowsMaxM * E)) return rc;
            if (int rc = dalloc(e, &ln.afrag, (size_t)kRowsMaxM * E)) return rc;
            if (int rc = dalloc(e, &ln.hfrag, (size_t)kRowsMaxM * 4 * E)) return rc;
            HIPCHK(e, hipMemset(ln.xfrag, 0, (size_t)kRowsMaxM * E * 4));
            HIPCHK(e, hipMemset(ln.afrag, 0, (size_t)kRowsMaxM * E * 4));
            HIPCHK(e, hipMemset(ln.hfrag, 0, (size_t)kRowsMaxM * 4 * E * 4));
        }
        HIPCHK(e, hipEventCreateWithFlags(&e->ev_lane_fork, hipEventDisableTiming));
    }
    if (int rc = dalloc(e, &e->dv.logits, 3 * Bm * 8192)) return rc;
    if (int rc = dalloc(e, &e->dv.logits_tar, Bm * kNBox * (size_t)cfg->bbox3d_vocab)) return rc;
    e->kv_scene_stride = (long)e->Lmax * 2 * E;
    e->kv_layer_stride = (long)Bm * e->kv_scene_stride;
    if (int rc = dev_alloc(e, &e->dv.kvcache, (size_t)cfg->n_oar_layer * e->kv_layer_stride * e->tsz)) return rc;
    // (the engines' key loops request whole 16-key passes and mask the keys past the step: p = 0 times whatever bits lie there must be 0, not NaN)
    HIPCHK(e, hipMemset(e->dv.kvcache, 0, (size_t)cfg->n_oar_layer * e->kv_layer_stride * e->tsz));
    // slot caches of the overlapped TAR pass: k | v rows of every temporal sub-block, all history slots (the foreground's growing-window
    // reuse allocates the same caches on first use, run_frame)
    if (e->overlap && !ensure_tcache(e)) e->overlap = false;     // keep the plain path rather than crowding the KV caches out
    if (const char* gc = getenv("UMGEN_GROW_CACHE")) e->grow_cache = gc[0] != '0';
    if (int rc = dalloc(e, &e->d_pose, Bm * Tm * 3)) return rc;
    if (int rc = dalloc(e, &e->d_pose_shift, Bm * Tm * 3)) return rc;
    if (int rc = dalloc(e, &e->d_map, Bm * Tm * kNMap)) return rc;
    if (int rc = dalloc(e, &e->d_box, Bm * Tm * kNBox)) return rc;
    if (int rc = dalloc(e, &e->d_img, Bm * Tm * kNImg)) return rc;
    if (int rc = dalloc(e, &e->dv.d_tokens, Bm * kTokPerFrame)) return rc;
    if (int rc = dalloc(e, &e->dv.d_prev_box, Bm * kNBox)) return rc;
    if (int rc = dalloc(e, &e->d_forced, Bm * kTokPerFrame)) return rc;
    if (int rc = dalloc(e, &e->d_counters, (size_t)8)) return rc;
    if (int rc = dalloc(e, &e->dv.d_nboxes, Bm)) return rc;
    if (int rc = dalloc(e, &e->d_ego_tok, Bm * 3)) return rc;
    if (int rc = dalloc(e, &e->d_item_scene, Bm)) return rc;
    if (int rc = dalloc(e, &e->dv.d_control, Bm * kSlots)) return rc;
    if (int rc = dalloc(e, &e->dv.d_boxes, Bm * 64 * 10)) return rc;
    if (int rc = dalloc(e, &e->dv.d_seeds, Bm)) return rc;
    if (int rc = dalloc(e, &e->dv.d_state, (size_t)1)) return rc;
    // the side outputs of the frame being generated, the call's bias tables and the samplers' scratch rows: with the engine, so that the step graphs
    // captured later hold these pointers
    int rc = 0;
    const auto side = [&](auto** p, size_t per_token) { if (!rc) rc = dalloc(e, p, Bm * kTokPerFrame * per_token); };
    DetailOut& d = e->dv.d_side.detail;
    side(&e->dv.d_side.logp, 1); side(&e->dv.d_side.logz, 1); side(&d.rank, 1); side(&d.mass_above, 1); side(&d.entropy, 1);
    side(&d.topk_tok, kDetailTopK); side(&d.topk_logp, kDetailTopK);
    if (rc) return rc;
    // (the pool holds the kBiasSetsMax table sets of a planned call; a call's one set is set 0 of it)
    DrawPlan& dp = e->dv.d_plan;
    lay_out_sets(dp, {cfg->pose_vocab, cfg->map_vocab, cfg->bbox3d_vocab, cfg->img_vocab});
    if (int rc = dalloc(e, &dp.pool, (size_t)kBiasSetsMax * dp.stride)) return rc;
    if (int rc = dalloc(e, &dp.rows, Bm * kBiasRows * kBiasRowLen)) return rc;
    if (int rc = dalloc(e, &dp.set_classes, (size_t)kBiasSetsMax)) return rc;
    if (int rc = dalloc(e, &dp.sp_of, Bm)) return rc;
    if (int rc = dalloc(e, &dp.set_of, Bm)) return rc;
    HIPCHK(e, hipMemset(dp.set_classes, 0, (size_t)kBiasSetsMax * sizeof(int)));
    HIPCHK(e, hipMemset(dp.set_of, 0xFF, Bm * sizeof(int)));
    return 0;
}

int alloc_engine_buffers(umgen_engine* e, const umgen_config* cfg) {
    const size_t Bm = cfg->max_batch;
    // ---- XCD-resident decode engine (UMGEN_DECODE_ENGINE=0 keeps the five-launch decode layer) ----
    if (e->eng_enabled) {
        if (int rc = dalloc(e, &e->d_layers, (size_t)cfg->n_oar_layer)) return rc;
        std::vector<OarLayerDev> hl(cfg->n_oar_layer);
        for (int i = 0; i < cfg->n_oar_layer; ++i) {
            const SubW& w = e->oar[i];
            hl[i] = OarLayerDev{reinterpret_cast<const bf16_t*>(w.attn.Wqkv), reinterpret_cast<const bf16_t*>(w.attn.Wo),
                                reinterpret_cast<const bf16_t*>(w.mlp.Wfc), reinterpret_cast<const bf16_t*>(w.mlp.Wproj), nullptr,
                                w.attn.bqkv, w.attn.bo, w.ln_a, w.ln_b};
        }
        HIPCHK(e, hipMemcpy(e->d_layers, hl.data(), hl.size() * sizeof(OarLayerDev), hipMemcpyHostToDevice));
        e->eng_gloc_bytes = (size_t)16 * kEngLocStride * 8;
        if (int rc = dalloc(e, &e->eng_gx, Bm * kEngE)) return rc;
        if (int rc = dev_alloc(e, reinterpret_cast<void**>(&e->eng_gloc), e->eng_gloc_bytes)) return rc;
        if (int rc = dalloc(e, &e->eng_ticket, (size_t)16)) return rc;
        if (int rc = dalloc(e, &e->eng_err, (size_t)4)) return rc;
        HIPCHK(e, hipMemset(e->eng_ticket, 0, 64));
        if (getenv("UMGEN_DEBUG_TIMING") && !e->bg_engine) {      // (per-phase stamps: the instantiation without background workers -- UMGEN_BG_ENGINE=0 for a one-scene engine)
            if (int rc = dalloc(e, &e->eng_stamps, (size_t)16)) return rc;
            HIPCHK(e, hipMemset(e->eng_stamps, 0, 128));
        }
        HIPCHK(e, hipMemset(e->eng_gx, 0, Bm * kEngE * 8));
        HIPCHK(e, hipMemset(e->eng_gloc, 0, e->eng_gloc_bytes));
        HIPCHK(e, hipMemset(e->eng_err, 0, 16));
        if (const char* bs = getenv("UMGEN_DEBUG_BURN")) {
            int us = 0, mf = 0, sl = 0, kb = 0;
            if (sscanf(bs, "%d,%d,%d,%d", &us, &mf, &sl, &kb) == 4 && kb > 0) {
                if (int rc = dev_alloc(e, &e->burn_buf, (size_t)kb << 10)) return rc;
                HIPCHK(e, hipMemset(e->burn_buf, 1, (size_t)kb << 10));
            }
        }
        if (getenv("UMGEN_DEBUG_TIMING")) fprintf(stderr, "[umgen] decode engine: on (8 XCD groups)\n");
    }
    if (e->wide_enabled) {
        if (int rc = dalloc(e, &e->d_layers_wide, (size_t)cfg->n_oar_layer)) return rc;
        if (int rc = dalloc(e, &e->wide_gran, oar_engine_wide_granules())) return rc;
        if (int rc = dalloc(e, &e->wide_ticket, (size_t)16)) return rc;      // one arrival counter per XCD
        if (int rc = dalloc(e, &e->wide_err, (size_t)4)) return rc;
        HIPCHK(e, hipMemset(e->wide_gran, 0, oar_engine_wide_granules() * 8));
        HIPCHK(e, hipMemset(e->wide_ticket, 0, 64));
        HIPCHK(e, hipMemset(e->wide_err, 0, 16));
        if (getenv("UMGEN_DEBUG_TIMING")) {
            if (int rc = dalloc(e, &e->wide_stamps, (size_t)16)) return rc;
            HIPCHK(e, hipMemset(e->wide_stamps, 0, 128));
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int umgen_create(const umgen_config* cfg, umgen_engine** out) {
    if (!cfg || !out) return UMGEN_E_INVALID;
    *out = nullptr;
    umgen_engine* e = new umgen_engine();
    *out = e;   // returned even on failure so the caller can read umgen_last_error()
    e->cfg = *cfg;
    if (int rc = validate_config(e, cfg)) return rc;
    // overlapped TAR pass (UMGEN_OVERLAP=0 disables it): the decode stream and the background stream get disjoint CU masks --
    // measured on MI355X, a decode loop sharing CUs with a concurrent GEMM stream runs at a quarter of its speed, with disjoint
    // masks (64 background CUs) it loses 8 %
    // The decode engine (oar_engine.hip) needs whole XCDs: 32 workgroups, one per CU, on each of them.  A CU mask cannot give
    // that -- measured with the engine's census: the mask bits are striped over the XCDs (64 background CUs = 8 CUs of EVERY
    // XCD), so a masked decode stream has 24 CUs per XCD.  The engine halves the decode loop, which is worth more than hiding the
    // TAR pass behind a launch-bound loop: when the engine can be used the overlap is off unless UMGEN_OVERLAP asks for it
    // (then the decode step is the five-launch form again).
    const CreateCtx cc{cfg, getenv("UMGEN_DECODE_ENGINE"), getenv("UMGEN_OVERLAP")};
    if (int rc = census_xcd_engine(e, cc)) return rc;
    if (int rc = census_wide_engine(e, cc)) return rc;
    if (int rc = choose_overlap(e, cc)) return rc;
    if (int rc = register_parameters(e, cfg)) return rc;
    if (int rc = alloc_workspace(e, cfg)) return rc;
    if (int rc = alloc_decode_buffers(e, cfg)) return rc;
    if (int rc = alloc_engine_buffers(e, cfg)) return rc;
    return UMGEN_OK;
}

int umgen_destroy(umgen_engine* e) {
    if (!e) return UMGEN_OK;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();   // every stream of this engine (decode, background, side, unmasked) is idle before anything is freed
    if (e->wide_stamps) {
        unsigned long long st[16];
        if (hipMemcpy(st, e->wide_stamps, 128, hipMemcpyDeviceToHost) == hipSuccess && st[15]) {
            const char* nm[14] = {"wait x", "LN + qkv rows", "wait qkv", "attention", "wait waves", "quarter out + wait quarters", "merge + wait att", "c_proj", "wait x'",
                                  "LN + c_fc + GELU", "wait waves", "mlp partial sums", "wait partial sums", "add partials"};
            fprintf(stderr, "[umgen] chip-wide decode engine, rank 0 wave 0, us per layer over %llu layers:", st[15]);
            double tot = 0;
            for (int p = 0; p < 14; ++p) { fprintf(stderr, " %s %.2f", nm[p], (double)st[p] / 100.0 / (double)st[15]); tot += (double)st[p] / 100.0 / (double)st[15]; }
            fprintf(stderr, " | total %.2f\n", tot);
        }
    }
    if (e->eng_stamps) {
        unsigned long long st[16];
        if (hipMemcpy(st, e->eng_stamps, 128, hipMemcpyDeviceToHost) == hipSuccess && st[10]) {
            const char* nm[10] = {"wait x", "qkv rows", "wait qkv", "attention", "wait partials", "c_proj", "wait x'", "c_fc + partial sums", "wait partial sums", "add partials"};
            fprintf(stderr, "[umgen] decode engine, group 0 rank 0, us per item over %llu items:", st[10]);
            double tot = 0;
            for (int p = 0; p < 10; ++p) { fprintf(stderr, " %s %.2f", nm[p], (double)st[p] / 100.0 / (double)st[10]); tot += (double)st[p] / 100.0 / (double)st[10]; }
            fprintf(stderr, " (c_fc part %.2f)", (double)st[11] / 100.0 / (double)st[10]);
            fprintf(stderr, " | total %.2f\n", tot);
            if (st[15])
                fprintf(stderr, "[umgen] decode engine, prologue of a launch (%llu launches): kernel entry -> rank, step, epoch known %.2f us; kernel entry -> first item's q|k|v + parked mlp rows there %.2f us"
                        "; kernel entry -> first item's x, LN weights and q|k|v rows there %.2f us\n", st[15], (double)st[12] / 100.0 / (double)st[15],
                        (double)st[13] / 100.0 / (double)st[15], (double)st[14] / 100.0 / (double)st[15]);
        }
    }
    for (auto& row : e->step_graph)
        for (auto& g : row)
            if (g) hipGraphExecDestroy(g);
    for (auto& ln : e->lane) {
        for (auto& row : ln.graph)
            for (auto& g : row)
                if (g) hipGraphExecDestroy(g);
        if (ln.s) { hipStreamSynchronize(ln.s); hipStreamDestroy(ln.s); }
        if (ln.done) hipEventDestroy(ln.done);
    }
    if (e->ev_lane_fork) hipEventDestroy(e->ev_lane_fork);
    for (void* p : e->allocs) hipFree(p);
    for (auto& ev : e->ev) if (ev) hipEventDestroy(ev);
    for (auto& pr : e->gemm_ev) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto& pr : e->attn_ev) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto& pr : e->layer_ev) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    if (e->tb.gmap) {}   // tables are in allocs
    if (e->bg_stream) { hipStreamSynchronize(e->bg_stream); hipStreamDestroy(e->bg_stream); }
    if (e->full_stream) hipStreamDestroy(e->full_stream);
    for (int i = 0; i < 2; ++i) {
        if (e->side_stream[i]) hipStreamDestroy(e->side_stream[i]);
        if (e->ev_side_done[i]) hipEventDestroy(e->ev_side_done[i]);
    }
    if (e->ev_side_in) hipEventDestroy(e->ev_side_in);
    for (hipEvent_t ev : {e->ev_tar_done, e->ev_bg_done, e->ev_bg0, e->ev_pre_done, e->ev_drain0, e->ev_drain1}) if (ev) hipEventDestroy(ev);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
    return UMGEN_OK;
}

}  // extern "C"
