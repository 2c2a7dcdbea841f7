// Kernel-level test hooks of frame assembly (frame.hip, rowops.hip; host pointers in, host pointers out): token embedding + map warp, LayerNorm,
// conditioning rows, first input, ego queries, the given-token prefix rows and their K/V move, the per-token step (fixed / sampled token with
// the bbox3d control flow) and the ego sampler.  Each goes through the product's launcher.  Outputs start as NaN (or as the caller's buffer
// where they are in / out) and carry guard bands; every token a launch may use as a table index is checked against the table's size on the
// host first.  Used only by tests/; never called by the product path.
#include "debug_util.h"

// host image of EmbedTables: fp32 tables and raw bf16 bits, with their row counts (spe has kSeq rows, egoe 3, axe 8, grid_posi 1024)
struct umgen_dbg_tables {
    const float *egoe, *axe, *be, *tpe, *spe, *gmap, *gimg;
    const uint16_t *fouier_pe, *posi, *grid_posi;
    int32_t E, n_tpe, n_pose, n_map, n_box, n_img, n_posi;
};

// everything umgen_dbg_token_steps reads and writes (see there)
struct umgen_dbg_steps {
    const float *cond, *logits, *logits_tar;
    const int32_t* prev_box;
    const unsigned char* control_slot;
    const int32_t* forced;
    const uint64_t* seeds;
    int32_t* tokens;
    float* x_next;
    int32_t *counters, *n_boxes;
    double* boxes;
    uint32_t* state_log;
    SamplerParams sp;
    int32_t B, j0, j1, given_end, ld_logits, use_forced, use_control, frame_idx;
    uint32_t epoch0;
};

namespace {
inline bool tables_sane(const umgen_dbg_tables* t) {
    return t && t->E >= 1 && t->n_tpe >= 0 && t->n_pose >= 0 && t->n_map >= 0 && t->n_box >= 0 && t->n_img >= 0 && t->n_posi >= 0;
}
// the tables a hook was given, on the device (an absent one stays nullptr)
EmbedTables tables_in(Scratch& s, const umgen_dbg_tables& t) {
    const size_t E = (size_t)t.E;
    EmbedTables tb{};
    tb.E = t.E;
    tb.egoe = s.in(t.egoe, 3 * E * 4);
    tb.axe = s.in(t.axe, 8 * E * 4);
    tb.be = s.in(t.be, (size_t)t.n_box * E * 4);
    tb.tpe = s.in(t.tpe, (size_t)t.n_tpe * E * 4);
    tb.spe = s.in(t.spe, (size_t)kSeq * E * 4);
    tb.gmap = s.in(t.gmap, (size_t)t.n_map * E * 4);
    tb.gimg = s.in(t.gimg, (size_t)t.n_img * E * 4);
    tb.fouier_pe = s.in(t.fouier_pe, (size_t)t.n_pose * E * 2);
    tb.posi = s.in(t.posi, (size_t)t.n_posi * E * 2);
    tb.grid_posi = s.in(t.grid_posi, (size_t)kNMap * E * 2);
    return tb;
}
// The side outputs of a sampler hook for n = B * 2199 positions (all in / out: a position no sampled step reaches keeps what it was handed): logp, logz
// [n] or NULL, and with `detail` the five arrays of the diagnostics, on the host [n] and [n][topk], on the device in the kernels' layout -- the lists
// kDetailTopK apart, the entries behind topk all bits set, and checked to come back that way.  d: the device bundle, a member not asked for null
struct SideHook {
    size_t n;
    float *logp = nullptr, *logz = nullptr;
    bool detail = false;
    int topk = 0;
    int32_t* rank = nullptr; float *mass_above = nullptr, *entropy = nullptr; int32_t* topk_tok = nullptr; float* topk_logp = nullptr;
    TokenSide d{};
    std::vector<uint32_t> wt{}, wl{};
    void ask_detail(int k, int32_t* r, float* ma, float* en, int32_t* tt, float* tl) { detail = true; topk = k; rank = r; mass_above = ma; entropy = en; topk_tok = tt; topk_logp = tl; }
    bool sane() const { return !detail || (rank && mass_above && entropy && topk >= 0 && topk <= kDetailTopK && (topk == 0 || (topk_tok && topk_logp))); }
    void widen(const void* host, std::vector<uint32_t>& w) const {
        w.assign(n * kDetailTopK, 0xffffffffu);
        for (size_t i = 0; i < n; ++i) memcpy(&w[i * kDetailTopK], (const uint32_t*)host + i * topk, (size_t)topk * 4);
    }
    void to_device(Scratch& s) {
        if (logp) d.logp = s.inout(logp, n * 4);
        if (logz) d.logz = s.inout(logz, n * 4);
        if (!detail) return;
        d.detail.rank = s.inout(rank, n * 4); d.detail.mass_above = s.inout(mass_above, n * 4); d.detail.entropy = s.inout(entropy, n * 4);
        if (!topk) return;
        widen(topk_tok, wt); widen(topk_logp, wl);
        d.detail.topk_tok = s.inout(wt.data(), wt.size() * 4); d.detail.topk_logp = s.inout(wl.data(), wl.size() * 4);
    }
    int narrow(void* host, const void* dev, std::vector<uint32_t>& w) const {
        if (down(w.data(), dev, w.size() * 4)) return UMGEN_E_HIP;
        for (size_t i = 0; i < n; ++i) {
            memcpy((uint32_t*)host + i * topk, &w[i * kDetailTopK], (size_t)topk * 4);
            for (int k = topk; k < kDetailTopK; ++k)
                if (w[i * kDetailTopK + k] != 0xffffffffu) return UMGEN_E_STATE;
        }
        return UMGEN_OK;
    }
    int to_host() {
        if ((logp && down(logp, d.logp, n * 4)) || (logz && down(logz, d.logz, n * 4))) return UMGEN_E_HIP;
        if (!detail) return UMGEN_OK;
        if (down(rank, d.detail.rank, n * 4) || down(mass_above, d.detail.mass_above, n * 4) || down(entropy, d.detail.entropy, n * 4)) return UMGEN_E_HIP;
        if (!topk) return UMGEN_OK;
        if (int rc = narrow(topk_tok, d.detail.topk_tok, wt)) return rc;
        return narrow(topk_logp, d.detail.topk_logp, wl);
    }
};
// The sampling plan of a hook on the host: sp_of [B] per-scene settings (NULL: OarState::plan bit 0 stays off); bias_set_of [B] (NULL: bit 1 stays off)
// with the pool of n_sets table sets and set_classes [n_sets], the class bits (1 << kBiasPose ..) of every set.  The tables of a biased hook are the plan
// of one set with bias_set_of all 0.
struct PlanHook {
    const SamplerParams* sp_of;
    const float* pool;
    int n_sets;
    const int32_t* set_classes;
    const int32_t* bias_set_of;
    int bits() const { return (sp_of ? kPlanSettings : 0) | (bias_set_of ? kPlanSets : 0); }
};
// How a set of a hook's pool lies (stride and class_off, by the engine's lay_out_sets), the class bits a set may carry, and the vocabularies of the classes
// the hook's sampler reads (0: not this sampler's class, its table is never checked).  The token-step hooks: the engine's layout, pose [3][n_pose] | map
// [n_map] | bbox3d [11][n_box] | image [n_img]; the ego hooks: pose [3][V]
struct SetLayout { long stride, class_off[4]; int classes, vocab[4]; };
inline SetLayout layout_of(const int (&vocab)[4], int classes, int read) {
    DrawPlan p{};
    lay_out_sets(p, vocab);
    SetLayout lay{p.stride, {}, classes, {}};
    for (int c = 0; c < 4; ++c) { lay.class_off[c] = p.class_off[c]; lay.vocab[c] = ((read >> c) & 1) ? vocab[c] : 0; }
    return lay;
}
inline SetLayout token_layout(const umgen_dbg_tables& t) { return layout_of({t.n_pose, t.n_map, t.n_box, t.n_img}, 15, 14); }
inline SetLayout ego_layout(int V) { return layout_of({V, 0, 0, 0}, 1 << kBiasPose, 1 << kBiasPose); }
inline bool sampler_params_sane(const SamplerParams& sp) {
    return sp.method >= 0 && sp.method <= 1 && sp.top_k >= 1 && sp.top_k_map >= 1 && sp.topk_image >= 1 && sp.temperature > 0.f;
}
int token_steps(const umgen_dbg_tables* t, const umgen_dbg_steps* a, SideHook& sh, const PlanHook* ph = nullptr);
// a hook's positions: B * 2199 (0 for a B the hook refuses anyway)
inline size_t side_n(int B) { return B < 1 ? 0 : (size_t)B * kTokPerFrame; }

// the body of umgen_dbg_embed_warp and umgen_dbg_embed_warp_slots (warped_all: nullptr, or the host buffer of launch_warp_map's output of that name)
int embed_warp(int stack, const umgen_dbg_tables* t, const int32_t* pose, const int32_t* map, const int32_t* box, const int32_t* img, int B, int T, int Tfull,
               int t0, const float* pose_diff, int want_last, float* X, float* mapfeat, float* warped_last, float* warped_all) {
    if (stack < STACK_EGO || stack > STACK_TAR || !tables_sane(t) || B < 1 || T < 1 || Tfull < 0 || t0 < 0) return UMGEN_E_INVALID;
    const int Tf = Tfull ? Tfull : T;
    if (t0 + T > Tf || Tf > t->n_tpe || !pose || !map || !box || !img || !pose_diff || !X || !mapfeat || !warped_last) return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->tpe || !t->spe || !t->gmap || !t->gimg || !t->fouier_pe || !t->posi || !t->grid_posi) return UMGEN_E_INVALID;
    const size_t F = (size_t)B * Tf, E = (size_t)t->E;
    if (!in_range(pose, F * kNPose, t->n_pose) || !in_range(map, F * kNMap, t->n_map) || !in_range(box, F * kNBox, t->n_box) ||
        !in_range(img, F * kNImg, t->n_img))
        return UMGEN_E_INVALID;
    for (size_t f = 0; f < F; ++f)
        for (int sl = 0; sl < kSlots; ++sl)
            if (box[f * kNBox + sl * kSlotLen] >= t->n_posi || box[f * kNBox + sl * kSlotLen + 1] >= t->n_posi) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * T * stack_len(stack) * E, mn = (size_t)B * T * kNMap * E, wn = (size_t)B * kNMap * E;
    Scratch s;
    const EmbedTables tb = tables_in(s, *t);
    WindowTokens w{};
    w.pose = s.in(pose, F * kNPose * 4); w.map = s.in(map, F * kNMap * 4); w.box = s.in(box, F * kNBox * 4); w.img = s.in(img, F * kNImg * 4);
    w.B = B; w.T = T; w.Tfull = Tfull; w.t0 = t0;
    const float* dPD = s.in(pose_diff, F * 3 * 4);
    float *dX = s.out(xn * 4), *dMF = s.out(mn * 4), *dWL = s.out(wn * 4), *dWA = nullptr;
    if (warped_all) dWA = s.out(mn * 4);
    if (s.rc) return s.rc;
    if (fill_nan(dX, xn, 0) || fill_nan(dMF, mn, 0) || fill_nan(dWL, wn, 0) || (dWA && fill_nan(dWA, mn, 0))) return UMGEN_E_HIP;
    launch_embed_stack(nullptr, stack, tb, w, dX, dMF);
    if (stack != STACK_EGO) launch_warp_map(nullptr, stack, tb, B, T, dMF, dPD, dX, want_last ? dWL : nullptr, Tfull, t0, dWA);
    if (int rc = s.finish()) return rc;
    if (down(X, dX, xn * 4) || down(mapfeat, dMF, mn * 4)) return UMGEN_E_HIP;
    if (dWA && down(warped_all, dWA, mn * 4)) return UMGEN_E_HIP;
    return down(warped_last, dWL, wn * 4);
}
}  // namespace

extern "C" {

// run_stack's first two launches (engine_stacks.hip): launch_embed_stack, then for every stack but STACK_EGO launch_warp_map.  Token arrays
// [B][Tf][3 | 1024 | 660 | 512] and pose_diff [B][Tf][3] with Tf = Tfull (0: T); the pass covers slots t0 .. t0 + T - 1.
// -> X [B][T][stack_len][E], mapfeat [B][T][1024][E], warped_last [B][1024][E] (handed to the launcher only when want_last != 0).
int umgen_dbg_embed_warp(int stack, const umgen_dbg_tables* t, const int32_t* pose, const int32_t* map, const int32_t* box, const int32_t* img, int B,
                         int T, int Tfull, int t0, const float* pose_diff, int want_last, float* X, float* mapfeat, float* warped_last) {
    return embed_warp(stack, t, pose, map, box, img, B, T, Tfull, t0, pose_diff, want_last, X, mapfeat, warped_last, nullptr);
}

// umgen_dbg_embed_warp with the warped map of EVERY slot of the pass beside warped_last (launch_warp_map's warped_all; every stack but STACK_EGO):
// -> also warped_all [B][T][1024][E]
int umgen_dbg_embed_warp_slots(int stack, const umgen_dbg_tables* t, const int32_t* pose, const int32_t* map, const int32_t* box, const int32_t* img, int B,
                               int T, int Tfull, int t0, const float* pose_diff, int want_last, float* X, float* mapfeat, float* warped_last,
                               float* warped_all) {
    if (stack == STACK_EGO || !warped_all) return UMGEN_E_INVALID;
    return embed_warp(stack, t, pose, map, box, img, B, T, Tfull, t0, pose_diff, want_last, X, mapfeat, warped_last, warped_all);
}

// launch_layernorm<T> (T by prec) on n_rows rows of x (row r at x + r * row_stride, E <= 1536 columns) -> out [out_rows][E] of T, out_rows >= n_rows:
// NaN at the launch, so rows >= n_rows come back as NaN
int umgen_dbg_layernorm(int prec, const float* x, long row_stride, long n_rows, int E, const float* w, void* out, long out_rows) {
    if (prec < 0 || prec > 2 || !x || !w || !out || E < 1 || E > 64 * 24 || row_stride < E || n_rows < 1 || out_rows < n_rows) return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, on = (size_t)out_rows * E;
    Scratch s;
    const float *dXi = s.in(x, (size_t)n_rows * row_stride * 4), *dW = s.in(w, (size_t)E * 4);
    void* dO = s.out(on * es);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dO, on, prec)) return rc;
    by_prec(prec, [&](auto tag) { launch_layernorm<decltype(tag)>(nullptr, dXi, row_stride, n_rows, E, dW, (decltype(tag)*)dO); });
    if (int rc = s.finish()) return rc;
    return down(out, dO, on * es);
}

// launch_cond_rows of one stack: X [B][T][stack_len][E], ln_w [E], warped_last [B][1024][E] or NULL (required for STACK_MAP) -> cond
// [B][kSeq][E], in / out: the launch changes the stack's own rows only
int umgen_dbg_cond_rows(int stack, int B, int T, int E, const float* X, const float* ln_w, const float* warped_last, float* cond) {
    if (stack < STACK_MAP || stack > STACK_TAR || B < 1 || T < 1 || E < 1 || !X || !ln_w || !cond || (stack == STACK_MAP && !warped_last)) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * T * stack_len(stack) * E, wn = (size_t)B * kNMap * E, cn = (size_t)B * kSeq * E;
    Scratch s;
    const float *dXi = s.in(X, xn * 4), *dW = s.in(ln_w, (size_t)E * 4), *dWL = s.in(warped_last, wn * 4);
    float* dC = s.inout(cond, cn * 4);
    if (s.rc) return s.rc;
    launch_cond_rows(nullptr, stack, B, T, E, dXi, dW, dWL, dC);
    if (int rc = s.finish()) return rc;
    return down(cond, dC, cn * 4);
}

// launch_cond_rows_slots of one stack: X [B][T][stack_len][E], ln_w [E], warped_all [B][T][1024][E] or NULL (required for STACK_MAP), items [n_items][2] =
// (scene, slot) -> cond_all [n_items][kSeq][E], in / out: the launch changes the stack's own rows only
int umgen_dbg_cond_rows_slots(int stack, int B, int T, int E, const float* X, const float* ln_w, const float* warped_all, const int32_t* items, int n_items,
                              float* cond_all) {
    if (stack < STACK_MAP || stack > STACK_TAR || B < 1 || T < 1 || E < 1 || n_items < 1 || !X || !ln_w || !items || !cond_all || (stack == STACK_MAP && !warped_all))
        return UMGEN_E_INVALID;
    for (int i = 0; i < n_items; ++i)      // the items index X and warped_all
        if (items[2 * i] < 0 || items[2 * i] >= B || items[2 * i + 1] < 0 || items[2 * i + 1] >= T) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * T * stack_len(stack) * E, wn = (size_t)B * T * kNMap * E, cn = (size_t)n_items * kSeq * E;
    Scratch s;
    const float *dXi = s.in(X, xn * 4), *dW = s.in(ln_w, (size_t)E * 4), *dWA = s.in(warped_all, wn * 4);
    const int* dI = s.in(items, (size_t)n_items * 2 * 4);
    float* dC = s.inout(cond_all, cn * 4);
    if (s.rc) return s.rc;
    launch_cond_rows_slots(nullptr, stack, T, E, dXi, dW, dWA, dI, n_items, dC);
    if (int rc = s.finish()) return rc;
    return down(cond_all, dC, cn * 4);
}

// launch_first_input: x [B][E] = row [E] + cond[b][0] (cond [B][kSeq][E])
int umgen_dbg_first_input(int B, int E, const float* row, const float* cond, float* x) {
    if (B < 1 || E < 1 || !row || !cond || !x) return UMGEN_E_INVALID;
    const size_t cn = (size_t)B * kSeq * E, xn = (size_t)B * E;
    Scratch s;
    const float *dR = s.in(row, (size_t)E * 4), *dC = s.in(cond, cn * 4);
    float* dXo = s.out(xn * 4);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dXo, xn, 0)) return rc;
    launch_first_input(nullptr, B, E, dR, dC, dXo);
    if (int rc = s.finish()) return rc;
    return down(x, dXo, xn * 4);
}

// launch_ego_queries: x [B][3][E] = (egoe[j] + spe[j]) + tpe[T - 1]
int umgen_dbg_ego_queries(const umgen_dbg_tables* t, int B, int T, float* x) {
    if (!tables_sane(t) || B < 1 || T < 1 || T > t->n_tpe || !t->egoe || !t->spe || !t->tpe || !x) return UMGEN_E_INVALID;
    const size_t xn = (size_t)B * 3 * t->E;
    Scratch s;
    const EmbedTables tb = tables_in(s, *t);
    float* dXo = s.out(xn * 4);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dXo, xn, 0)) return rc;
    launch_ego_queries(nullptr, tb, B, T, dXo);
    if (int rc = s.finish()) return rc;
    return down(x, dXo, xn * 4);
}

// launch_ego_queries with a window length per item: x [n][3][E] = (egoe[j] + spe[j]) + tpe[item_T[i] - 1]
int umgen_dbg_ego_queries_slots(const umgen_dbg_tables* t, int n, const int32_t* item_T, float* x) {
    if (!tables_sane(t) || n < 1 || !item_T || !t->egoe || !t->spe || !t->tpe || !x) return UMGEN_E_INVALID;
    for (int i = 0; i < n; ++i)
        if (item_T[i] < 1 || item_T[i] > t->n_tpe) return UMGEN_E_INVALID;
    const size_t xn = (size_t)n * 3 * t->E;
    Scratch s;
    const EmbedTables tb = tables_in(s, *t);
    const int* dT = s.in(item_T, (size_t)n * 4);
    float* dXo = s.out(xn * 4);
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dXo, xn, 0)) return rc;
    launch_ego_queries(nullptr, tb, n, 0, dXo, dT);
    if (int rc = s.finish()) return rc;
    return down(x, dXo, xn * 4);
}

// launch_prefix_rows: the decode inputs of the given positions 0 .. P - 1 (tske_row [E], cond [B][kSeq][E], tokens [B][2199]) ->
// X [B][P - 1][E] (rows 0 .. P - 2) and x_last [B][E] (row P - 1)
int umgen_dbg_prefix_rows(const umgen_dbg_tables* t, const float* tske_row, const float* cond, const int32_t* tokens, int B, int P, float* X, float* x_last) {
    if (!tables_sane(t) || B < 1 || P < 2 || P > kBoxEos + 2 || !tske_row || !cond || !tokens || !X || !x_last) return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->gmap || !t->fouier_pe) return UMGEN_E_INVALID;
    for (int b = 0; b < B; ++b) {
        const int32_t* tk = tokens + (size_t)b * kTokPerFrame;
        if (!in_range(tk, kNPose, t->n_pose) || !in_range(tk + kOffMap, kNMap, t->n_map) || !in_range(tk + kOffBox, kNBox, t->n_box)) return UMGEN_E_INVALID;
    }
    const size_t E = (size_t)t->E, cn = (size_t)B * kSeq * E, xn = (size_t)B * (P - 1) * E, ln = (size_t)B * E, tn = (size_t)B * kTokPerFrame;
    Scratch s;
    const EmbedTables tb = tables_in(s, *t);
    const float *dR = s.in(tske_row, E * 4), *dC = s.in(cond, cn * 4);
    const int* dT = s.in(tokens, tn * 4);
    float *dXo = s.out(xn * 4), *dL = s.out(ln * 4);
    if (s.rc) return s.rc;
    if (fill_nan(dXo, xn, 0) || fill_nan(dL, ln, 0)) return UMGEN_E_HIP;
    launch_prefix_rows(nullptr, tb, dR, dC, dT, B, P, dXo, dL);
    if (int rc = s.finish()) return rc;
    if (down(X, dXo, xn * 4)) return UMGEN_E_HIP;
    return down(x_last, dL, ln * 4);
}

// launch_prefix_kv_to_cache<T>: qk [B * S][2E] (q | k rows) and vt [B][H][48][S_pad] of T -> cache [B][2][H][Lmax][48] of T (NaN at the launch) with
// the product's scene stride 2 * H * Lmax * 48
int umgen_dbg_prefix_kv_to_cache(int prec, const void* qk, const void* vt, int B, int S, int S_pad, int H, int Lmax, void* cache) {
    if (prec < 0 || prec > 2 || !qk || !vt || !cache || B < 1 || S < 1 || S > S_pad || S > Lmax || H < 1) return UMGEN_E_INVALID;
    const size_t es = prec ? 2 : 4, E = (size_t)H * kHeadDim, qn = (size_t)B * S * 2 * E, vn = (size_t)B * E * S_pad, stride = (size_t)2 * H * Lmax * kHeadDim;
    const size_t cn = (size_t)B * stride;
    Scratch s;
    const void *dQ = s.in(qk, qn * es), *dV = s.in(vt, vn * es);
    void* dC = s.out(cn * es, scene_band(stride * es, B));
    if (s.rc) return s.rc;
    if (int rc = fill_nan(dC, cn, prec)) return rc;
    by_prec(prec, [&](auto tag) {
        typedef decltype(tag) TT;
        launch_prefix_kv_to_cache<TT>(nullptr, (const TT*)dQ, (const TT*)dV, B, S, S_pad, H, Lmax, (TT*)dC, (long)stride);
    });
    if (int rc = s.finish()) return rc;
    return down(cache, dC, cn * es);
}

// The sampler kernels of decode steps j0 .. j1 - 1 of one frame for B scenes, on an OarState and a SampleArgs of the hook's own: what enqueue_step
// (engine_decode.hip) launches behind the head at position j -- launch_fixed_token for bos / eos / the pose prefix and every position < given_end,
// else launch_sample_token with the position's mod and vocabulary (tables: n_map | n_box | n_img) -- with that step's logits [B][ld_logits]
// (logits [j1 - j0][B][ld_logits]).  logits_tar [B][660][n_box], prev_box [B][660], control_slot [B][60], forced [B][2199] (or NULL), seeds [B].
// In / out: tokens [B][2199], counters [8], n_boxes [B], boxes [B][64][10].  Out: x_next [j1 - j0][B][E] (NaN before every step) and
// state_log [j1 - j0][3] = OarState step, epoch, done behind every step.
int umgen_dbg_token_steps(const umgen_dbg_tables* t, const umgen_dbg_steps* a) {
    SideHook sh{side_n(a ? a->B : 0)};
    return token_steps(t, a, sh);
}
// The same with OarState::want_logp = 1 and SampleArgs::side.logp = logp [B][2199] (in / out: the sampled steps write their position, nothing else changes)
int umgen_dbg_token_steps_logp(const umgen_dbg_tables* t, const umgen_dbg_steps* a, float* logp) {
    SideHook sh{side_n(a ? a->B : 0), logp};
    return logp ? token_steps(t, a, sh) : UMGEN_E_INVALID;
}
// ... and with OarState::want_detail = 1, detail_topk = topk and SampleArgs::side.detail = rank, mass_above, entropy [B][2199], topk_tok, topk_logp [B][2199][topk]
// (in / out like logp; the lists may be NULL when topk == 0)
int umgen_dbg_token_steps_detail(const umgen_dbg_tables* t, const umgen_dbg_steps* a, float* logp, int topk, int32_t* rank, float* mass_above,
                                 float* entropy, int32_t* topk_tok, float* topk_logp) {
    if (!logp || !a || a->B < 1) return UMGEN_E_INVALID;
    SideHook sh{side_n(a->B), logp};
    sh.ask_detail(topk, rank, mass_above, entropy, topk_tok, topk_logp);
    return sh.sane() ? token_steps(t, a, sh) : UMGEN_E_INVALID;
}
// ... and with the logit-bias tables of a biased call: bias_map [n_map], bias_box [11][n_box], bias_img [n_img] (any may be NULL; entries finite or -inf,
// every row with an allowed entry) are the one set of a plan that puts every scene on set 0 (OarState::plan = kPlanSets), DrawPlan::rows is the hook's
// scratch; logz [B][2199] (in / out, or NULL) sets want_logz.  logp may be NULL
static int token_steps_biased(const umgen_dbg_tables* t, const umgen_dbg_steps* a, SideHook& sh, const float* bias_map, const float* bias_box,
                              const float* bias_img) {
    if (!tables_sane(t) || !a || a->B < 1 || std::max(t->n_map, std::max(t->n_box, t->n_img)) > 8192) return UMGEN_E_INVALID;
    const SetLayout lay = token_layout(*t);
    const float* const tab[4] = {nullptr, bias_map, bias_box, bias_img};
    std::vector<float> pool((size_t)lay.stride, NAN);      // (a class without a table is never read: NaN would show)
    const std::vector<int32_t> set_of((size_t)a->B, 0);
    int32_t classes = 0;
    for (int c = kBiasMap; c <= kBiasImg; ++c)
        if (tab[c]) { memcpy(pool.data() + lay.class_off[c], tab[c], (size_t)kPlanTableRows[c] * lay.vocab[c] * 4); classes |= 1 << c; }
    const PlanHook ph{nullptr, pool.data(), 1, &classes, set_of.data()};
    return token_steps(t, a, sh, &ph);
}
int umgen_dbg_token_steps_biased(const umgen_dbg_tables* t, const umgen_dbg_steps* a, float* logp, const float* bias_map, const float* bias_box,
                                 const float* bias_img, float* logz) {
    SideHook sh{side_n(a ? a->B : 0), logp, logz};
    return token_steps_biased(t, a, sh, bias_map, bias_box, bias_img);
}
// ... together with umgen_dbg_token_steps_detail's diagnostics (they stay on the unbiased row)
int umgen_dbg_token_steps_biased_detail(const umgen_dbg_tables* t, const umgen_dbg_steps* a, float* logp, const float* bias_map, const float* bias_box,
                                        const float* bias_img, float* logz, int topk, int32_t* rank, float* mass_above, float* entropy, int32_t* topk_tok,
                                        float* topk_logp) {
    if (!logp || !a || a->B < 1) return UMGEN_E_INVALID;
    SideHook sh{side_n(a->B), logp, logz};
    sh.ask_detail(topk, rank, mass_above, entropy, topk_tok, topk_logp);
    return sh.sane() ? token_steps_biased(t, a, sh, bias_map, bias_box, bias_img) : UMGEN_E_INVALID;
}
// ... and under a sampling plan (OarState::plan) in the place of the three tables: sp_of [B] per-scene settings (or NULL: a->sp for every scene), and
// bias_set_of [B] (or NULL: no tables), scene b's set in the pool of n_sets sets (-1: none), with set_classes [n_sets]; a set lies like the engine's,
// pose [3][n_pose] | map [n_map] | bbox3d [11][n_box] | image [n_img], the sets back to back.  Both NULL: the switch stays 0
int umgen_dbg_token_steps_planned(const umgen_dbg_tables* t, const umgen_dbg_steps* a, float* logp, float* logz, int topk, int32_t* rank, float* mass_above,
                                  float* entropy, int32_t* topk_tok, float* topk_logp, const SamplerParams* sp_of, const float* pool, int n_sets,
                                  const int32_t* set_classes, const int32_t* bias_set_of) {
    if (!logp || !a || a->B < 1) return UMGEN_E_INVALID;
    const PlanHook ph{sp_of, pool, n_sets, set_classes, bias_set_of};
    SideHook sh{side_n(a->B), logp, logz};
    sh.ask_detail(topk, rank, mass_above, entropy, topk_tok, topk_logp);
    return sh.sane() ? token_steps(t, a, sh, &ph) : UMGEN_E_INVALID;
}

}  // extern "C"

namespace {
// every row of a bias table: finite or -inf entries, one of them allowed
bool bias_rows_sane(const float* tab, int rows, int V) {
    for (int r = 0; tab && r < rows; ++r) {
        int allowed = 0;
        for (int n = 0; n < V; ++n) {
            const float v = tab[(size_t)r * V + n];
            if (v != v || v == INFINITY) return false;
            allowed += v != -INFINITY;
        }
        if (!allowed) return false;
    }
    return true;
}
// a hook's plan: settings a sampler takes, sets within the pool, scenes within the sets, every set's bits among lay.classes and its tables of the hook's
// classes like bias_rows_sane
bool plan_sane(const PlanHook& ph, int B, const SetLayout& lay) {
    for (int b = 0; ph.sp_of && b < B; ++b)
        if (!sampler_params_sane(ph.sp_of[b])) return false;
    if (!ph.bias_set_of) return true;
    if (ph.n_sets < 0 || ph.n_sets > kBiasSetsMax || (ph.n_sets > 0 && (!ph.pool || !ph.set_classes))) return false;
    for (int b = 0; b < B; ++b)
        if (ph.bias_set_of[b] < -1 || ph.bias_set_of[b] >= ph.n_sets) return false;
    for (int q = 0; q < ph.n_sets; ++q) {
        const int cl = ph.set_classes[q];
        if (cl & ~lay.classes) return false;
        for (int c = 0; c < 4; ++c)
            if (((cl >> c) & 1) && lay.vocab[c] && !bias_rows_sane(ph.pool + (size_t)q * lay.stride + lay.class_off[c], kPlanTableRows[c], lay.vocab[c])) return false;
    }
    return true;
}
// ... on the device: the samplers' DrawPlan, with scratch rows when it has sets
DrawPlan plan_to_device(Scratch& s, const PlanHook& ph, int B, const SetLayout& lay) {
    DrawPlan p{};
    p.sp_of = s.in(ph.sp_of, (size_t)B * sizeof(SamplerParams));
    if (!ph.bias_set_of) return p;
    int32_t classes[kBiasSetsMax] = {};
    for (int q = 0; q < ph.n_sets; ++q) classes[q] = ph.set_classes[q];
    p.set_classes = s.in(classes, sizeof(classes));
    p.set_of = s.in(ph.bias_set_of, (size_t)B * 4);
    p.pool = s.in(ph.pool, (size_t)ph.n_sets * lay.stride * 4);      // (no set: nullptr, and no scene reads it)
    p.stride = lay.stride;
    for (int c = 0; c < 4; ++c) p.class_off[c] = lay.class_off[c];
    p.rows = s.out((size_t)B * kBiasRows * kBiasRowLen * 4);
    return p;
}
int token_steps(const umgen_dbg_tables* t, const umgen_dbg_steps* a, SideHook& sh, const PlanHook* ph) {
    if (!tables_sane(t) || !a || a->B < 1 || a->j0 < 0 || a->j1 <= a->j0 || a->j1 > kImgEos) return UMGEN_E_INVALID;
    // given tokens end behind the pose prefix, the map or the boxes (umgen_frame's given_end): fixed_token_kernel knows no given image token
    if (a->given_end != kPoseEos + 1 && a->given_end != kMapEos + 1 && a->given_end != kBoxEos + 1) return UMGEN_E_INVALID;
    if (!a->cond || !a->logits || !a->logits_tar || !a->prev_box || !a->control_slot || !a->seeds || !a->tokens || !a->x_next || !a->counters ||
        !a->n_boxes || !a->boxes || !a->state_log || (a->use_forced && !a->forced))
        return UMGEN_E_INVALID;
    if (!t->axe || !t->be || !t->gmap || !t->gimg || !t->fouier_pe || t->E > 6 * 256) return UMGEN_E_INVALID;   // CondRow: E <= 1536
    const int vmax = std::max(t->n_map, std::max(t->n_box, t->n_img));
    if (vmax > 8192 || a->ld_logits < vmax || t->n_map < 1 || t->n_img < 1 || t->n_box <= kBoxPad) return UMGEN_E_INVALID;
    if (a->sp.method < 0 || a->sp.method > 1 || a->sp.top_k < 1 || a->sp.top_k_map < 1 || a->sp.topk_image < 1 || !(a->sp.temperature > 0.f)) return UMGEN_E_INVALID;
    const int B = a->B, n = a->j1 - a->j0;
    for (int b = 0; b < B; ++b) {
        const int32_t* tk = a->tokens + (size_t)b * kTokPerFrame;
        if (!in_range(tk, kNPose, t->n_pose) || !in_range(tk + kOffMap, kNMap, t->n_map) || !in_range(tk + kOffBox, kNBox, t->n_box) ||
            !in_range(tk + kOffImg, kNImg, t->n_img))
            return UMGEN_E_INVALID;
        if (a->use_forced) {
            const int32_t* ft = a->forced + (size_t)b * kTokPerFrame;
            if (!in_range(ft, kNPose, t->n_pose)) return UMGEN_E_INVALID;
            if (!in_range(ft + kOffMap, kNMap, t->n_map) || !in_range(ft + kOffBox, kNBox, t->n_box) || !in_range(ft + kOffImg, kNImg, t->n_img)) return UMGEN_E_INVALID;
        }
        if (a->n_boxes[b] < 0 || a->n_boxes[b] > 30) return UMGEN_E_INVALID;     // the kernel's box list and corner table hold 64
    }
    const size_t E = (size_t)t->E, cn = (size_t)B * kSeq * E, ln = (size_t)B * a->ld_logits, tarn = (size_t)B * kNBox * t->n_box, tn = (size_t)B * kTokPerFrame;
    const size_t bn = (size_t)B * 64 * 10, xn = (size_t)B * E;
    OarState s0{};
    s0.step = a->j0; s0.frame_idx = a->frame_idx; s0.use_forced = a->use_forced ? 1 : 0; s0.use_control = a->use_control ? 1 : 0; s0.done = 0;
    s0.epoch = a->epoch0; s0.sp = a->sp; s0.want_logp = sh.logp ? 1 : 0;
    s0.want_detail = sh.detail ? 1 : 0; s0.detail_topk = sh.topk; s0.want_logz = sh.logz ? 1 : 0;
    // a plan: the pool in the engine's layout
    const SetLayout lay = token_layout(*t);
    if (ph) {
        if (!plan_sane(*ph, B, lay)) return UMGEN_E_INVALID;
        s0.plan = ph->bits();
    }
    Scratch s;
    SampleArgs sa{};
    sa.tb = tables_in(s, *t);
    sa.st = s.in(&s0, sizeof(s0));
    float* dLg = s.raw(ln * 4);                 // the current step's logits
    sa.logits = dLg; sa.logits_tar = s.in(a->logits_tar, tarn * 4); sa.ld_logits = a->ld_logits; sa.ld_tar = t->n_box; sa.cond = s.in(a->cond, cn * 4);
    sa.prev_box = s.in(a->prev_box, (size_t)B * kNBox * 4); sa.control_slot = s.in(a->control_slot, (size_t)B * kSlots);
    sa.seeds = s.in(a->seeds, (size_t)B * 8);
    if (a->use_forced) sa.forced = s.in(a->forced, tn * 4); else sa.forced = s.raw(tn * 4);   // never read without use_forced
    sa.x_next = s.out(xn * 4); sa.tokens = s.inout(a->tokens, tn * 4); sa.counters = s.inout(a->counters, 8 * 4);
    sa.n_boxes = s.inout(a->n_boxes, (size_t)B * 4); sa.boxes = s.inout(a->boxes, bn * 8);
    sh.to_device(s);
    sa.side = sh.d;
    if (ph) sa.plan = plan_to_device(s, *ph, B, lay);
    if (s.rc) return s.rc;
    for (int i = 0; i < n; ++i) {
        const int j = a->j0 + i, mod = kind_of_pos(j, a->given_end);
        if (int rc = fill_nan(sa.x_next, xn, 0)) return rc;
        if (mod == 0) {
            launch_fixed_token(nullptr, sa, B);
        } else {
            if (up(dLg, a->logits + (size_t)i * ln, ln * 4)) return UMGEN_E_HIP;
            sa.mod = mod;
            sa.vocab = mod == 1 ? t->n_map : (mod == 2 ? t->n_box : t->n_img);
            launch_sample_token(nullptr, sa, B);
        }
        if (int rc = finish()) return rc;
        OarState s1{};
        if (down(&s1, sa.st, sizeof(s1)) || down(a->x_next + (size_t)i * xn, sa.x_next, xn * 4)) return UMGEN_E_HIP;
        a->state_log[3 * i] = (uint32_t)s1.step; a->state_log[3 * i + 1] = s1.epoch; a->state_log[3 * i + 2] = (uint32_t)s1.done;
    }
    if (!s.intact()) return UMGEN_E_STATE;
    if (down(a->tokens, sa.tokens, tn * 4) || down(a->counters, sa.counters, 8 * 4) || down(a->n_boxes, sa.n_boxes, (size_t)B * 4)) return UMGEN_E_HIP;
    if (int rc = sh.to_host()) return rc;
    return down(a->boxes, sa.boxes, bn * 8);
}
}  // namespace

extern "C" {

// launch_sample_ego: logits [3 B][V] -> out_tokens [B][3]; the draw of row (b, jq) is rng_uniform(seeds[b], frame_idx, kSeq + jq, DRAW_MAIN); forced
// [B][2199] (or NULL) overrides with its pose tokens.  logp [B][2199] (in / out, or NULL): entry [b][jq] receives the log-likelihood of pose token jq
// of scene b on its row
static int sample_ego_hook(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                           int32_t* out_tokens, SideHook& sh, const PlanHook* ph = nullptr) {
    const SetLayout lay = ego_layout(V);
    if (ph && (B < 1 || V < 1 || !plan_sane(*ph, B, lay))) return UMGEN_E_INVALID;
    if (!logits || !sp || !seeds || !out_tokens || B < 1 || V < 1 || V > 8192 || sp->method < 0 || sp->method > 1 || sp->top_k < 1 || !(sp->temperature > 0.f))
        return UMGEN_E_INVALID;
    for (int b = 0; (sh.logp || sh.detail) && forced && b < B; ++b)      // the scored token indexes the row
        if (!in_range(forced + (size_t)b * kTokPerFrame, kNPose, V)) return UMGEN_E_INVALID;
    const size_t ln = (size_t)B * 3 * V, tn = (size_t)B * kTokPerFrame, osz = (size_t)B * 3 * 4;
    Scratch s;
    const float* dL = s.in(logits, ln * 4);
    const unsigned long long* dS = s.in(seeds, (size_t)B * 8);
    const int* dF = s.in(forced, tn * 4);
    int *dOv = s.raw(4), *dT = s.out(osz);
    sh.to_device(s);
    EgoSide es{sh.d, sh.topk};
    if (ph) { es.plan_bits = ph->bits(); es.plan = plan_to_device(s, *ph, B, lay); }
    if (s.rc) return s.rc;
    if (hipMemset(dOv, 0, 4) != hipSuccess || hipMemset(dT, 0xff, osz) != hipSuccess) return UMGEN_E_HIP;
    launch_sample_ego(nullptr, dL, V, *sp, dS, frame_idx, dF, dT, B, dOv, es);
    if (int rc = finish()) return rc;
    int ovf = 0;
    if (down(&ovf, dOv, 4)) return UMGEN_E_HIP;
    if (!s.intact() || ovf != 0) return UMGEN_E_STATE;      // (the overflow word is unused since the exhaustive tie walk: it must stay 0)
    if (int rc = sh.to_host()) return rc;
    return down(out_tokens, dT, osz);
}
// the same with a pose bias table bias [3][V] (or NULL) and logz [B][2199] (in / out, or NULL): entries [b][jq].  The table is the one set of a plan that
// puts every scene on set 0; no table, no plan
int umgen_dbg_sample_ego_biased(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                                int32_t* out_tokens, const float* bias, float* logp, float* logz) {
    SideHook sh{side_n(B), logp, logz};
    if (!bias) return sample_ego_hook(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, sh);
    if (B < 1) return UMGEN_E_INVALID;
    const std::vector<int32_t> set_of((size_t)B, 0);
    const int32_t classes = 1 << kBiasPose;
    const PlanHook ph{nullptr, bias, 1, &classes, set_of.data()};
    return sample_ego_hook(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, sh, &ph);
}
// the same under a sampling plan: sp_of [B] (or NULL: *sp for every scene); bias_set_of [B] (or NULL) into a pool of n_sets pose tables [n_sets][3][V] with
// set_classes [n_sets] (bit kBiasPose: the set has its table); rank .. topk_logp: umgen_dbg_sample_ego_detail's diagnostics (rank NULL: none), every
// scene's mass_above at its own temperature
int umgen_dbg_sample_ego_planned(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                                 int32_t* out_tokens, float* logp, float* logz, int topk, int32_t* rank, float* mass_above, float* entropy,
                                 int32_t* topk_tok, float* topk_logp, const SamplerParams* sp_of, const float* pool, int n_sets,
                                 const int32_t* set_classes, const int32_t* bias_set_of) {
    const PlanHook ph{sp_of, pool, n_sets, set_classes, bias_set_of};
    SideHook sh{side_n(B), logp, logz};
    if (rank) sh.ask_detail(topk, rank, mass_above, entropy, topk_tok, topk_logp);      // (rank NULL: no diagnostics, like umgen_dbg_sample_ego_biased)
    if (!sh.sane() || (sh.detail && !logp)) return UMGEN_E_INVALID;
    return sample_ego_hook(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, sh, &ph);
}
int umgen_dbg_sample_ego_logp(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                              int32_t* out_tokens, float* logp) {
    SideHook sh{side_n(B), logp};
    return sample_ego_hook(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, sh);
}
// the same with the diagnostics of the three pose tokens: rank, mass_above, entropy [B][2199], topk_tok, topk_logp [B][2199][topk] (in / out, entries [b][jq])
int umgen_dbg_sample_ego_detail(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                                int32_t* out_tokens, float* logp, int topk, int32_t* rank, float* mass_above, float* entropy, int32_t* topk_tok,
                                float* topk_logp) {
    if (B < 1) return UMGEN_E_INVALID;
    SideHook sh{side_n(B), logp};
    sh.ask_detail(topk, rank, mass_above, entropy, topk_tok, topk_logp);
    return sh.sane() ? sample_ego_hook(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, sh) : UMGEN_E_INVALID;
}
int umgen_dbg_sample_ego(const float* logits, int V, const SamplerParams* sp, const uint64_t* seeds, int frame_idx, const int32_t* forced, int B,
                         int32_t* out_tokens) {
    return umgen_dbg_sample_ego_logp(logits, V, sp, seeds, frame_idx, forced, B, out_tokens, nullptr);
}

}  // extern "C"
