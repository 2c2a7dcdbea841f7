// Host side of a generated token's side outputs, plain C++ (no HIP, no engine types): beside its token a decode step can leave the token's log-likelihood
// (logp), logz of a biased call, and its diagnostics (rank, mass_above, entropy, top-K lists).  On the device they are one bundle of [B][2199] buffers
// (TokenSide, frame.h); here are the host buffers of one frame in that layout (FrameSide), their owner for a whole call with the scatter into the
// caller's arrays (GenSide), and the list of (device, host, bytes) a frame fills and copies back (side_buffers).  umgen_frame_biased and the rollout
// driver (engine.hip) build one GenSide per call; tests/host/gen_side_test.cpp holds deliver and side_buffers to element-by-element indexing.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#include "token_windows.h"

namespace umgen {

constexpr int kSideTopK = 16;   // list entries per position in the device layout (kDetailTopK, frame.h)

// Host buffers of one frame's side outputs in the device layout: [B][2199], the lists [B][2199][kSideTopK] with the first topk entries of a position
// written.  A null member is not asked for; rank, mass_above and entropy come together (rank stands for the three), the lists only with topk > 0
struct FrameSide {
    float *logp, *logz;
    int* rank; float *mass_above, *entropy;
    int* topk_tok; float* topk_logp;
    int topk;
};

// The caller's arrays of a generation call, one [4] group per output in the modality order (what MOD4 yields of the ABI's output structs): every group
// [items][S_mod], the lists [items][S_mod][topk]; any pointer may be null
struct SideDst {
    float *logp[4], *logz[4];
    int* rank[4]; float *mass_above[4], *entropy[4];
    int* topk_tok[4]; float* topk_logp[4];
    int topk;
    template <typename P> static bool any(P* const (&g)[4]) { return g[0] || g[1] || g[2] || g[3]; }
    bool wants_lists() const { return any(topk_tok) || any(topk_logp); }
    bool wants_detail() const { return any(rank) || any(mass_above) || any(entropy) || wants_lists(); }
};

// The side outputs of a call over `items` scenes: the frame buffers, sized from what the caller asked for, and their way into the caller's arrays
struct GenSide {
    SideDst dst{};      // topk is 0 when nobody receives a list (lists nobody receives are not formed)
    std::vector<float> f_logp, f_logz, f_mass, f_ent, f_tlp;
    std::vector<int> f_rank, f_tok;
    FrameSide fs{};

    void init(const SideDst& d, size_t items) {
        dst = d;
        if (!d.wants_lists()) dst.topk = 0;
        const size_t n = items * kFrameRowLen, det = d.wants_detail() ? n : 0, lists = dst.topk ? n * kSideTopK : 0;
        f_logp.resize(SideDst::any(d.logp) ? n : 0); f_logz.resize(SideDst::any(d.logz) ? n : 0);
        f_rank.resize(det); f_mass.resize(det); f_ent.resize(det);
        f_tok.resize(lists); f_tlp.resize(lists);
        const auto ptr = [](auto& v) { return v.empty() ? nullptr : v.data(); };
        fs = FrameSide{ptr(f_logp), ptr(f_logz), ptr(f_rank), ptr(f_mass), ptr(f_ent), ptr(f_tok), ptr(f_tlp), dst.topk};
    }
    const FrameSide* frame() const { return fs.logp || fs.logz || fs.rank ? &fs : nullptr; }
    // scene b of the frame just generated -> item `item` of the caller's arrays
    void deliver(size_t b, size_t item) const {
        const size_t topk = (size_t)dst.topk;
        for (int m = 0; m < 4; ++m) {
            const size_t src = b * kFrameRowLen + kModOff[m], at = item * kModLen[m], len = (size_t)kModLen[m];
            if (dst.logp[m]) memcpy(dst.logp[m] + at, &f_logp[src], len * sizeof(float));
            if (dst.logz[m]) memcpy(dst.logz[m] + at, &f_logz[src], len * sizeof(float));
            if (dst.rank[m]) memcpy(dst.rank[m] + at, &f_rank[src], len * sizeof(int));
            if (dst.mass_above[m]) memcpy(dst.mass_above[m] + at, &f_mass[src], len * sizeof(float));
            if (dst.entropy[m]) memcpy(dst.entropy[m] + at, &f_ent[src], len * sizeof(float));
            for (size_t i = 0; i < len && topk; ++i) {
                if (dst.topk_tok[m]) memcpy(dst.topk_tok[m] + (at + i) * topk, &f_tok[(src + i) * kSideTopK], topk * sizeof(int));
                if (dst.topk_logp[m]) memcpy(dst.topk_logp[m] + (at + i) * topk, &f_tlp[(src + i) * kSideTopK], topk * sizeof(float));
            }
        }
    }
};

// What a frame of B scenes fills with 0xFF before its first step -- NaN / -1 wherever no head runs -- and copies back behind its last: (device pointer,
// host pointer, bytes) of the members the call asked for, in the order logp, logz, rank, mass_above, entropy, topk_tok, topk_logp.  Dev is TokenSide
// (frame.h); a template only so that this header, and its test, stay free of HIP
struct SideBuf { void* dev; void* host; size_t bytes; };
struct SideBufs {
    SideBuf buf[7];
    int n = 0;
    const SideBuf* begin() const { return buf; }
    const SideBuf* end() const { return buf + n; }
};
template <typename Dev>
SideBufs side_buffers(const Dev& d, const FrameSide& h, size_t B) {
    const size_t bytes = B * kFrameRowLen * 4;
    SideBufs s;
    if (h.logp) s.buf[s.n++] = SideBuf{d.logp, h.logp, bytes};
    if (h.logz) s.buf[s.n++] = SideBuf{d.logz, h.logz, bytes};
    if (h.rank) {
        s.buf[s.n++] = SideBuf{d.detail.rank, h.rank, bytes};
        s.buf[s.n++] = SideBuf{d.detail.mass_above, h.mass_above, bytes};
        s.buf[s.n++] = SideBuf{d.detail.entropy, h.entropy, bytes};
        if (h.topk > 0) {
            s.buf[s.n++] = SideBuf{d.detail.topk_tok, h.topk_tok, bytes * kSideTopK};
            s.buf[s.n++] = SideBuf{d.detail.topk_logp, h.topk_logp, bytes * kSideTopK};
        }
    }
    return s;
}

}  // namespace umgen
