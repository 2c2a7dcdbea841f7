// Host token windows, plain C++ (no HIP): a scene's tokens as one per-modality view (TokenView) or owner (TokenSeqs), the one gather that cuts
// windows of w frames out of per-item sequences (gather_windows), the packing of frames into [2199] rows (frame_rows), the int64 -> int32
// narrowing at the ABI boundary (narrow_tokens) and the window rule of rollout, clip and futures (cond_window).  Every host pass of the
// engine_*.hip files stages its uploads through these; tests/host/token_windows_test.cpp holds them to element-by-element indexing.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace umgen {

// the four modalities of a frame in the order pose | map | bbox3d | image: content length, and offset in a frame's [2199] row
constexpr int kModLen[4] = {3, 1024, 660, 512}, kModOff[4] = {0, 3, 1027, 1687};
constexpr int kFrameRowLen = 2199;

// Host int32 tokens of `items` sequences of `frames` frames, not owned: mod[m] is [items][frames][kModLen[m]]
struct TokenView {
    const int* mod[4];
    int frames;
    const int* at(int m, size_t item, size_t frame) const { return mod[m] + (item * (size_t)frames + frame) * kModLen[m]; }
    const int* pose() const { return mod[0]; }
};

// ... and owned.  A view of it is valid until the next resize
struct TokenSeqs {
    std::vector<int> mod[4];
    int frames = 0;
    void resize(size_t items, int frames_per_item) {
        frames = frames_per_item;
        for (int m = 0; m < 4; ++m) mod[m].resize(items * (size_t)frames * kModLen[m]);
    }
    int* at(int m, size_t item, size_t frame) { return mod[m].data() + (item * (size_t)frames + frame) * kModLen[m]; }
    TokenView view() const { return TokenView{{mod[0].data(), mod[1].data(), mod[2].data(), mod[3].data()}, frames}; }
};

// The window rule of umgen_rollout, umgen_score_clip and umgen_score_futures (UMGen.py:1597-1603; Engine.clip_windows / future_windows): frame f of
// a sequence is conditioned on the n = min(f, cond) frames before it, [start, start + n)
struct CondWindow { int start, n; };
inline CondWindow cond_window(int f, int cond) {
    const int n = std::min(f, cond);
    return CondWindow{f - n, n};
}

// frames [at, at + count) of items [0, n) of `out`, which its owner has sized: item i takes frames [first(i), first(i) + count) of item source(i) of `in`
template <typename Source, typename First>
void copy_frames(const TokenView& in, size_t n, Source source, First first, int count, TokenSeqs& out, int at) {
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < n && count > 0; ++i)
            memcpy(out.at(m, i, (size_t)at), in.at(m, (size_t)source(i), (size_t)first(i)), (size_t)count * kModLen[m] * sizeof(int));
}
// out = n windows of w frames, [n][w][S_mod]: window i is frames [first(i), first(i) + w) of item source(i) of `in`
template <typename Source, typename First>
void gather_windows(const TokenView& in, size_t n, Source source, First first, int w, TokenSeqs& out) {
    out.resize(n, w);
    copy_frames(in, n, source, first, w, out, 0);
}
// ... every item its own window, all from frame `start`
inline void gather_windows(const TokenView& in, size_t n, int start, int w, TokenSeqs& out) {
    gather_windows(in, n, [](size_t i) { return i; }, [start](size_t) { return start; }, w, out);
}
// ... items [i0, i0 + n) of a fan of C items per source item: item i reads source item i / C
inline void gather_fan_windows(const TokenView& in, size_t i0, size_t n, int C, int start, int w, TokenSeqs& out) {
    gather_windows(in, n, [i0, C](size_t i) { return (i0 + i) / (size_t)C; }, [start](size_t) { return start; }, w, out);
}

// rows [n][2199] pose | map | bbox3d | image: row i is frame frame(i) of item source(i) of `in`
template <typename Source, typename Frame>
void frame_rows(const TokenView& in, size_t n, Source source, Frame frame, int* rows) {
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < n; ++i) memcpy(rows + i * kFrameRowLen + kModOff[m], in.at(m, (size_t)source(i), (size_t)frame(i)), (size_t)kModLen[m] * sizeof(int));
}

// int64 tokens [items][frames][S_mod] of every modality, as the ABI takes them, as int32
inline void narrow_tokens(const int64_t* const in[4], size_t items, int frames, TokenSeqs& out) {
    out.resize(items, frames);
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < out.mod[m].size(); ++i) out.mod[m][i] = (int)in[m][i];
}

}  // namespace umgen
