// Weights and constant tables: umgen_load_tensor, umgen_finalize_weights (the bf16 tables, the GMLP rows, the decode engines' repacked
// layers) and the numpy-faithful host arithmetic behind them and behind the pose shift.
#include "engine_state.h"

namespace {

// ---- numpy-faithful host helpers (unfused double arithmetic) ----------------------------------------------
#pragma clang fp contract(off)
double lin_bin(int i, double start, double stop, int n) {   // np.linspace(start, stop, n)[i]
    if (i >= n - 1) return stop;
    const double step = (stop - start) / (double)(n - 1);
    volatile double t = (double)i * step;
    return t + start;
}
// UMGen.decode_pose (UMGen.py:1008-1024): DigitalBinsTokenizer.decode + Normalize_Standard.unnormalize_ego
float decode_pose_value(int tok, int axis) {
    const float stdv[3] = {10.0f, 4.0f, 1.0f};
    const float inv_std = 1.0f / stdv[axis];                 // np.float32 division (normalize.py:26)
    const int right = std::min(std::max(tok, 0), 1023), left = std::min(std::max(tok - 1, 0), 1023);
    volatile double s = lin_bin(left, -1.0, 1.0, 1024) + lin_bin(right, -1.0, 1.0, 1024);
    volatile double v = s / 2.0;
    volatile double u = v / (double)inv_std;
    return (float)(u + 0.0);
}
// module.py:746-768 position_encoding_init -> bf16
void sinusoid_table(int n_position, int E, int start_index, std::vector<bf16_t>& out) {
    out.assign((size_t)n_position * E, 0);
    for (int pos = 1; pos < n_position; ++pos)
        for (int j = 0; j < E; ++j) {
            const double denom = std::pow(10000.0, 2.0 * (double)(j / 2) / (double)E);
            const double a = (double)(pos + start_index) / denom;
            const double v = (j % 2 == 0) ? std::sin(a) : std::cos(a);
            // double -> bf16 round-to-nearest-even (via the exactly-representable float when possible)
            float f = (float)v;
            // correct double rounding: if the float rounding moved across a bf16 tie, fix it up
            bf16_t b = f32_to_bf16(f);
            const double lo = (double)bf16_to_f32((bf16_t)(b - 1)), hi = (double)bf16_to_f32((bf16_t)(b + 1)), mid = (double)bf16_to_f32(b);
            // choose nearest of the three candidates to v (ties to even mantissa)
            double best = mid;
            bf16_t bb = b;
            const double cands[2] = {lo, hi};
            const bf16_t cb[2] = {(bf16_t)(b - 1), (bf16_t)(b + 1)};
            for (int c = 0; c < 2; ++c) {
                const double d1 = std::fabs(cands[c] - v), d0 = std::fabs(best - v);
                if (d1 < d0 || (d1 == d0 && (cb[c] & 1) == 0 && (bb & 1) == 1)) { best = cands[c]; bb = cb[c]; }
            }
            out[(size_t)pos * E + j] = bb;
        }
}

template <typename T> void convert_to(const void* src, int dtype, size_t n, T* dst);
float load_as_f32(const void* src, int dtype, size_t i) {
    switch (dtype) {
        case UMGEN_DT_F32: return reinterpret_cast<const float*>(src)[i];
        case UMGEN_DT_BF16: return bf16_to_f32(reinterpret_cast<const bf16_t*>(src)[i]);
        case UMGEN_DT_F64: return (float)reinterpret_cast<const double*>(src)[i];
        case UMGEN_DT_F16: {
            const uint16_t h = reinterpret_cast<const uint16_t*>(src)[i];
            const uint32_t sign = (h >> 15) & 1, ex = (h >> 10) & 31, man = h & 1023;
            float v;
            if (ex == 0) v = std::ldexp((float)man, -24);
            else if (ex == 31) v = man ? NAN : INFINITY;
            else v = std::ldexp((float)(man | 1024), (int)ex - 25);
            return sign ? -v : v;
        }
    }
    return 0.f;
}

// Decode engine (oar_engine.hip): the mlp c_proj of every BlockOAR, repacked for the hidden-unit split.  CU c of a group owns
// hidden units 96 c .. 96 c + 95; thread t of its workgroup holds, as 16-byte units of 8 bf16 in the order it requests them, the matrix-core
// A fragments of its wave: unit f = 3 tile + kstep of lane (t % 64) of wave (t / 64) is
//   W[96 wave + 16 tile + lane % 16][96 c + 32 kstep + 8 (lane / 16) .. + 7]
// layout [32 CUs][18 units][512 threads][8]: a wave's request of one unit is 1 KB contiguous.
int repack_mlp_proj(umgen_engine* e) {
    const int E = e->E, F4 = 4 * E;
    std::vector<bf16_t> src((size_t)E * F4), dst((size_t)kEngGroup * kEngWpUnits * kEngThreads * 8);
    std::vector<OarLayerDev> hl(e->oar.size());
    HIPCHK(e, hipMemcpy(hl.data(), e->d_layers, hl.size() * sizeof(OarLayerDev), hipMemcpyDeviceToHost));
    if (e->eng_wp2.size() != e->oar.size()) {
        e->eng_wp2.assign(e->oar.size(), nullptr);
        for (auto& p : e->eng_wp2)
            if (int rc = dev_alloc(e, &p, dst.size() * sizeof(bf16_t))) return rc;
    }
    for (size_t li = 0; li < e->oar.size(); ++li) {
        HIPCHK(e, hipMemcpy(src.data(), e->oar[li].mlp.Wproj, src.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (int c = 0; c < kEngGroup; ++c)
            for (int j = 0; j < kEngWpUnits; ++j)
                for (int t = 0; t < kEngThreads; ++t) {
                    bf16_t* d8 = &dst[(((size_t)c * kEngWpUnits + j) * kEngThreads + t) * 8];
                    const int wave = t / 64, lane = t % 64, tile = j / 3, ks = j % 3;
                    memcpy(d8, &src[(size_t)(96 * wave + 16 * tile + lane % 16) * F4 + 96 * c + 32 * ks + 8 * (lane / 16)], 8 * sizeof(bf16_t));
                }
        HIPCHK(e, hipMemcpy(e->eng_wp2[li], dst.data(), dst.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
        hl[li].Wp2 = reinterpret_cast<const bf16_t*>(e->eng_wp2[li]);
        {
            // c_fc [4E][E] as the engine's A fragments: CU c owns rows 96 c .. + 95 (6 tiles of 16), wave v the k range 96 v .. + 95
            // (3 k-steps of 32); fragment f = 3 tile + kstep of lane l = W[96 c + 16 tile + l % 16][96 v + 32 kstep + 8 (l / 16) .. + 7],
            // stored [c][v][f][l][8]: a wave's request of one fragment is 1 KB contiguous (row-strided 64-byte pieces streamed at
            // two thirds of the rate where the weight stream is not hidden: 4 scenes 564 vs 511 us per launch)
            if (e->eng_wf2.size() != e->oar.size()) e->eng_wf2.assign(e->oar.size(), nullptr);
            std::vector<bf16_t> fsrc((size_t)F4 * E), fdst((size_t)F4 * E);
            if (!e->eng_wf2[li])
                if (int rc = dev_alloc(e, &e->eng_wf2[li], fdst.size() * sizeof(bf16_t))) return rc;
            HIPCHK(e, hipMemcpy(fsrc.data(), e->oar[li].mlp.Wfc, fsrc.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
            for (int c = 0; c < kEngGroup; ++c)
                for (int v = 0; v < 8; ++v)
                    for (int f = 0; f < 18; ++f)
                        for (int ln = 0; ln < 64; ++ln)
                            memcpy(&fdst[((((size_t)c * 8 + v) * 18 + f) * 64 + ln) * 8],
                                   &fsrc[(size_t)(96 * c + 16 * (f / 3) + ln % 16) * E + 96 * v + 32 * (f % 3) + 8 * (ln / 16)], 8 * sizeof(bf16_t));
            HIPCHK(e, hipMemcpy(e->eng_wf2[li], fdst.data(), fdst.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
            hl[li].Wf2 = reinterpret_cast<const bf16_t*>(e->eng_wf2[li]);
        }
    }
    HIPCHK(e, hipMemcpy(e->d_layers, hl.data(), hl.size() * sizeof(OarLayerDev), hipMemcpyHostToDevice));
    return 0;
}

// Layer table of the chip-wide engine (oar_engine_wide.hip) + its mlp c_proj slices: rank r multiplies its 24 hidden units h[24 r ..] into ALL E
// output rows, so its slice is W[row][24 r .. 24 r + 23] for every row: [256 ranks][E rows][24], 48 contiguous bytes per (rank, row).
int repack_wide(umgen_engine* e) {
    const int E = e->E, F4 = 4 * E, RF = F4 / kWideGroups;
    std::vector<bf16_t> src((size_t)E * F4), dst((size_t)E * F4);
    std::vector<OarLayerDev> hl(e->oar.size());
    if (e->wide_wp2.size() != e->oar.size()) {
        e->wide_wp2.assign(e->oar.size(), nullptr);
        for (auto& p : e->wide_wp2)
            if (int rc = dev_alloc(e, &p, dst.size() * sizeof(bf16_t))) return rc;
    }
    for (size_t li = 0; li < e->oar.size(); ++li) {
        const SubW& w = e->oar[li];
        HIPCHK(e, hipMemcpy(src.data(), w.mlp.Wproj, src.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (int r = 0; r < kWideGroups; ++r)
            for (int row = 0; row < E; ++row)
                memcpy(&dst[((size_t)r * E + row) * RF], &src[(size_t)row * F4 + (size_t)RF * r], RF * sizeof(bf16_t));
        HIPCHK(e, hipMemcpy(e->wide_wp2[li], dst.data(), dst.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
        hl[li] = OarLayerDev{reinterpret_cast<const bf16_t*>(w.attn.Wqkv), reinterpret_cast<const bf16_t*>(w.attn.Wo),
                             reinterpret_cast<const bf16_t*>(w.mlp.Wfc), reinterpret_cast<const bf16_t*>(w.mlp.Wproj),
                             reinterpret_cast<const bf16_t*>(e->wide_wp2[li]), w.attn.bqkv, w.attn.bo, w.ln_a, w.ln_b, nullptr};
    }
    HIPCHK(e, hipMemcpy(e->d_layers_wide, hl.data(), hl.size() * sizeof(OarLayerDev), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

namespace umgen {

void decode_pose_shift(const int* pose, const int* ego, int B, int Tn, std::vector<int>& pshift, std::vector<float>& pdiff) {
    // pose shifted one frame ahead (UMGen.py:1445-1452) and its decoded (dx, dy, dtheta) for the map warp
    pshift.resize((size_t)B * Tn * 3);
    pdiff.resize((size_t)B * Tn * 3);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < Tn; ++t)
            for (int a = 0; a < 3; ++a) {
                const int v = (t + 1 < Tn) ? pose[((size_t)b * Tn + t + 1) * 3 + a] : ego[b * 3 + a];
                pshift[((size_t)b * Tn + t) * 3 + a] = v;
                pdiff[((size_t)b * Tn + t) * 3 + a] = decode_pose_value(v, a);
            }
}

}  // namespace umgen

extern "C" {

int umgen_load_tensor(umgen_engine* e, const char* key, const void* data, int32_t dtype, const int64_t* shape, int32_t ndim) {
    if (!e || !key || !data) return UMGEN_E_INVALID;
    auto it = e->slots.find(key);
    if (it == e->slots.end()) return 1;   // not consumed by the rollout (e.g. head_tar_pose, *.scale buffers)
    Slot& s = it->second;
    if ((size_t)ndim != s.shape.size()) return e->fail(UMGEN_E_INVALID, "%s: ndim %d, expected %zu", key, ndim, s.shape.size());
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != s.shape[i]) return e->fail(UMGEN_E_INVALID, "%s: dim %d is %lld, expected %lld", key, i, (long long)shape[i], (long long)s.shape[i]);
        n *= (size_t)shape[i];
    }
    if (dtype < 0 || dtype > UMGEN_DT_F64) return e->fail(UMGEN_E_INVALID, "%s: dtype %d", key, dtype);
    const bool to_bf16 = (s.kind == 2) || (s.kind == 1 && e->cfg.precision == UMGEN_PREC_BF16);
    if (s.kind == 1 && e->cfg.precision == UMGEN_PREC_FP16) {   // round-to-nearest-even to IEEE half, like torch's .half()
        std::vector<f16_t> h(n);
        if (dtype == UMGEN_DT_F16) memcpy(h.data(), data, n * 2);
        else {
            unsigned overflow = 0;                              // (no early exit in the conversion loop: it stays vectorisable)
            for (size_t i = 0; i < n; ++i) {
                const float v = load_as_f32(data, dtype, i);
                const uint16_t hb = f32_to_f16_bits_host(v);
                // the CONVERTED value decides, like torch's .half(): (65504, 65520) still rounds to 65504, only >= 65520 becomes inf
                overflow |= (unsigned)(((hb & 0x7fffu) == 0x7c00u) & (std::fabs(v) <= 3.4e38f));
                memcpy(&h[i], &hb, 2);
            }
            if (overflow) {                                     // a finite weight would become inf: refuse rather than decode garbage
                for (size_t i = 0; i < n; ++i) {
                    const float v = load_as_f32(data, dtype, i);
                    if (std::isfinite(v) && (f32_to_f16_bits_host(v) & 0x7fffu) == 0x7c00u)
                        return e->fail(UMGEN_E_INVALID, "%s[%zu] = %g does not fit fp16 (precision fp16 needs |w| < 65520)", key, i, (double)v);
                }
            }
        }
        HIPCHK(e, hipMemcpy(s.dst, h.data(), n * 2, hipMemcpyHostToDevice));
    } else if (to_bf16) {
        std::vector<bf16_t> h(n);
        if (dtype == UMGEN_DT_BF16) memcpy(h.data(), data, n * 2);
        else for (size_t i = 0; i < n; ++i) h[i] = f32_to_bf16(load_as_f32(data, dtype, i));
        HIPCHK(e, hipMemcpy(s.dst, h.data(), n * 2, hipMemcpyHostToDevice));
    } else {
        if (dtype == UMGEN_DT_F32) {
            HIPCHK(e, hipMemcpy(s.dst, data, n * 4, hipMemcpyHostToDevice));
        } else {
            std::vector<float> h(n);
            for (size_t i = 0; i < n; ++i) h[i] = load_as_f32(data, dtype, i);
            HIPCHK(e, hipMemcpy(s.dst, h.data(), n * 4, hipMemcpyHostToDevice));
        }
    }
    s.loaded = true;
    e->finalized = false;
    return UMGEN_OK;
}

int umgen_finalize_weights(umgen_engine* e) {
    if (!e) return UMGEN_E_INVALID;
    std::string missing;
    int nmiss = 0;
    for (auto& kv : e->slots)
        if (!kv.second.loaded && !kv.second.optional) {
            if (nmiss < 4) missing += (nmiss ? ", " : "") + kv.first;
            ++nmiss;
        }
    if (nmiss) return e->fail(UMGEN_E_STATE, "%d state-dict entries not loaded (e.g. %s)", nmiss, missing.c_str());
    const int E = e->E;
    std::vector<bf16_t> posi;
    const bool have_posi = e->slots["bbox3d_spatial_posi"].loaded;
    if (!e->slots["fouier_pe"].loaded) {
        std::vector<bf16_t> t;
        sinusoid_table(1024, E, 0, t);
        HIPCHK(e, hipMemcpy(const_cast<bf16_t*>(e->tb.fouier_pe), t.data(), t.size() * 2, hipMemcpyHostToDevice));
    }
    if (!have_posi) {
        sinusoid_table(1030, E, 1024, posi);
        HIPCHK(e, hipMemcpy(const_cast<bf16_t*>(e->tb.posi), posi.data(), posi.size() * 2, hipMemcpyHostToDevice));
    } else {
        posi.resize((size_t)1030 * E);
        HIPCHK(e, hipMemcpy(posi.data(), e->tb.posi, posi.size() * 2, hipMemcpyDeviceToHost));
    }
    if (!e->slots["grid_center_posi_embedding"].loaded) {
        // UMGen.py:140-153, 357-383: token of grid centre c = 62 - 4g is np.digitize((c + 64)/128, linspace(0,1,1024))
        std::vector<bf16_t> gp((size_t)1024 * E);
        int tok[32];
        for (int g = 0; g < 32; ++g) {
            const double x = ((double)(62 - 4 * g) + 64.0) / 128.0;
            int c = 0;
            for (int i = 0; i < 1024; ++i) if (lin_bin(i, 0.0, 1.0, 1024) <= x) ++c;
            tok[g] = c;
        }
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j)
                for (int c = 0; c < E; ++c)
                    gp[((size_t)i * 32 + j) * E + c] = f32_to_bf16(bf16_to_f32(posi[(size_t)tok[i] * E + c]) + bf16_to_f32(posi[(size_t)tok[j] * E + c]));
        HIPCHK(e, hipMemcpy(const_cast<bf16_t*>(e->tb.grid_posi), gp.data(), gp.size() * 2, hipMemcpyHostToDevice));
    }
    const int rc = build_tables_any(e, Place{e->stream, &e->w_main});
    if (rc) return rc;
    if (e->eng_enabled) { if (int rc2 = repack_mlp_proj(e)) return rc2; }
    if (e->wide_enabled) { if (int rc2 = repack_wide(e)) return rc2; }
    e->px.valid = false;   // slot caches filled with other weights are not a prefix of anything
    e->finalized = true;
    return UMGEN_OK;
}

}  // extern "C"
