// Host test of umgen_amd/csrc/token_windows.h (started by tests/test_token_windows_host.py; no GPU, no HIP): gather_windows / copy_frames, frame_rows,
// narrow_tokens and cond_window against element-by-element indexing, and for B = 2 scenes of N = 3 branches and every (T_in, new_frames, cond) in
// {1,2,3} x {0..4} x {1,2,3} the window sequence of the rollout driver -- one conditioning sequence, cond_window, one gather per frame, reading scene
// i / N of the caller's arrays -- against a literal transcription of the slide / append sequence it replaced, run on explicitly replicated inputs, with a
// control-box overwrite at one frame that has to survive a slide.
#include <cstdio>
#include <cstdlib>

#include "token_windows.h"

using namespace umgen;

static int g_fail = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (++g_fail <= 20) { printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                                              \
    } while (0)

// a token that names its place: every (modality, item, frame, position) its own value
static int tok(int m, size_t item, size_t frame, int k) { return (int)(((item * 131 + frame) * 4 + m) * 1024 + k); }
static TokenSeqs make_seqs(size_t items, int frames, int salt = 0) {
    TokenSeqs s;
    s.resize(items, frames);
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < items; ++i)
            for (int t = 0; t < frames; ++t)
                for (int k = 0; k < kModLen[m]; ++k) s.mod[m][((i * frames) + t) * kModLen[m] + k] = tok(m, i + salt, t, k);
    return s;
}

static void test_layout() {
    CHECK(kModOff[0] == 0 && kModOff[1] == kModLen[0] && kModOff[2] == kModOff[1] + kModLen[1] && kModOff[3] == kModOff[2] + kModLen[2], "offsets");
    CHECK(kFrameRowLen == kModOff[3] + kModLen[3] && kFrameRowLen == 2199, "row length %d", kFrameRowLen);
    const TokenSeqs s = make_seqs(3, 4);
    const TokenView v = s.view();
    CHECK(v.frames == 4 && v.pose() == s.mod[0].data(), "view");
    for (int m = 0; m < 4; ++m) {
        CHECK(s.mod[m].size() == (size_t)3 * 4 * kModLen[m], "size of modality %d", m);
        for (size_t i = 0; i < 3; ++i)
            for (size_t t = 0; t < 4; ++t) CHECK(v.at(m, i, t)[kModLen[m] - 1] == tok(m, i, t, kModLen[m] - 1), "at(%d, %zu, %zu)", m, i, t);
    }
}

static void test_cond_window() {
    for (int cond = 1; cond <= 5; ++cond)
        for (int f = 1; f <= 9; ++f) {
            const CondWindow w = cond_window(f, cond);
            CHECK(w.n == (f < cond ? f : cond) && w.start == f - w.n && w.start >= 0 && w.start + w.n == f, "f %d cond %d -> start %d n %d", f, cond, w.start, w.n);
        }
}

static void test_gather() {
    const TokenSeqs src = make_seqs(5, 6);
    TokenSeqs out;
    // every index term: a source map that is not the identity, per-item starts, w from 0 to the whole sequence
    for (int w = 0; w <= 6; ++w) {
        const size_t n = 7;
        const auto source = [](size_t i) { return (i * 3 + 1) % 5; };
        const auto first = [w](size_t i) { return (int)(i % (size_t)(6 - w + 1)); };
        gather_windows(src.view(), n, source, first, w, out);
        CHECK(out.frames == w, "frames %d", out.frames);
        for (int m = 0; m < 4; ++m) {
            CHECK(out.mod[m].size() == n * w * kModLen[m], "w %d modality %d size", w, m);
            for (size_t i = 0; i < n; ++i)
                for (int t = 0; t < w; ++t)
                    for (int k = 0; k < kModLen[m]; ++k)
                        CHECK(out.mod[m][(i * w + t) * kModLen[m] + k] == tok(m, source(i), first(i) + t, k), "w %d m %d i %zu t %d k %d", w, m, i, t, k);
        }
    }
    // the same start for all items
    gather_windows(src.view(), 5, 2, 3, out);
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < 5; ++i)
            for (int t = 0; t < 3; ++t)
                for (int k = 0; k < kModLen[m]; ++k) CHECK(out.view().at(m, i, t)[k] == tok(m, i, 2 + t, k), "same start m %d i %zu t %d k %d", m, i, t, k);
    // a chunk [i0, i0 + n) of a fan of C items per source item
    gather_fan_windows(src.view(), 4, 9, 3, 1, 4, out);
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < 9; ++i)
            for (int t = 0; t < 4; ++t)
                for (int k = 0; k < kModLen[m]; ++k) CHECK(out.view().at(m, i, t)[k] == tok(m, (4 + i) / 3, 1 + t, k), "fan m %d i %zu t %d k %d", m, i, t, k);
    // copy_frames into the middle of sized items leaves the rest alone
    TokenSeqs dst = make_seqs(4, 5, 50);
    copy_frames(src.view(), 4, [](size_t i) { return 4 - i; }, [](size_t i) { return (int)i; }, 2, dst, 1);
    for (int m = 0; m < 4; ++m)
        for (size_t i = 0; i < 4; ++i)
            for (int t = 0; t < 5; ++t)
                for (int k = 0; k < kModLen[m]; ++k) {
                    const int want = (t == 1 || t == 2) ? tok(m, 4 - i, i + (t - 1), k) : tok(m, i + 50, t, k);
                    CHECK(dst.view().at(m, i, t)[k] == want, "copy_frames m %d i %zu t %d k %d", m, i, t, k);
                }
    copy_frames(src.view(), 4, [](size_t) { return 99; }, [](size_t) { return 99; }, 0, dst, 5);      // nothing to copy: nothing is addressed
}

static void test_frame_rows_and_narrow() {
    const TokenSeqs src = make_seqs(3, 4);
    const size_t n = 5;
    std::vector<int> rows(n * kFrameRowLen + 1, -7);
    const auto source = [](size_t i) { return (i * 2) % 3; };
    const auto frame = [](size_t i) { return (int)((i + 1) % 4); };
    frame_rows(src.view(), n, source, frame, rows.data());
    CHECK(rows[n * kFrameRowLen] == -7, "frame_rows wrote past its rows");
    for (size_t i = 0; i < n; ++i)
        for (int m = 0; m < 4; ++m)
            for (int k = 0; k < kModLen[m]; ++k) CHECK(rows[i * kFrameRowLen + kModOff[m] + k] == tok(m, source(i), frame(i), k), "row %zu m %d k %d", i, m, k);
    std::vector<int64_t> wide[4];
    const int64_t* in[4];
    for (int m = 0; m < 4; ++m) {
        wide[m].assign(src.mod[m].begin(), src.mod[m].end());
        in[m] = wide[m].data();
    }
    TokenSeqs back;
    narrow_tokens(in, 3, 4, back);
    CHECK(back.frames == 4, "narrow frames");
    for (int m = 0; m < 4; ++m) CHECK(back.mod[m] == src.mod[m], "narrow modality %d", m);
}

// ---- the rollout driver's windows ----------------------------------------------------------------------------------------------------------------

// what frame idx "generates" for item i, and what a control box writes over position k of the last conditioning frame (k % 7 == 0)
static int generated(int idx, int i, int m, int k) { return 900000 + ((idx * 16 + i) * 4 + m) * 1024 + k; }
static int control_box(int i, int k) { return -1000 - i * 1024 - k; }

// The sequence as it was written before: per modality a window vector that slides (keep the last cond frames) and is rebuilt with one more frame per
// item behind every frame; the control overwrite goes to its last box frame.  Runs on BN scenes: the replicated input.  Returns every frame's windows.
static std::vector<TokenSeqs> windows_slide_append(const TokenSeqs& in, int BN, int T_in, int new_frames, int cond, int ctl_frame) {
    std::vector<int> hist[4];
    for (int m = 0; m < 4; ++m) hist[m] = in.mod[m];
    int T_cur = T_in;
    std::vector<TokenSeqs> seen;
    for (int idx = 0; idx < new_frames; ++idx) {
        if (T_cur > cond) {
            for (int m = 0; m < 4; ++m) {
                std::vector<int> nw((size_t)BN * cond * kModLen[m]);
                for (int b = 0; b < BN; ++b)
                    memcpy(&nw[(size_t)b * cond * kModLen[m]], &hist[m][((size_t)b * T_cur + (T_cur - cond)) * kModLen[m]], (size_t)cond * kModLen[m] * sizeof(int));
                hist[m].swap(nw);
            }
            T_cur = cond;
        }
        if (idx == ctl_frame)
            for (int b = 0; b < BN; ++b)
                for (int k = 0; k < kModLen[2]; k += 7) hist[2][((size_t)b * T_cur + (T_cur - 1)) * kModLen[2] + k] = control_box(b, k);
        TokenSeqs w;
        w.frames = T_cur;
        for (int m = 0; m < 4; ++m) w.mod[m] = hist[m];
        seen.push_back(w);
        for (int m = 0; m < 4; ++m) {
            std::vector<int> nw((size_t)BN * (T_cur + 1) * kModLen[m]);
            for (int b = 0; b < BN; ++b) {
                memcpy(&nw[(size_t)b * (T_cur + 1) * kModLen[m]], &hist[m][(size_t)b * T_cur * kModLen[m]], (size_t)T_cur * kModLen[m] * sizeof(int));
                for (int k = 0; k < kModLen[m]; ++k) nw[((size_t)b * (T_cur + 1) + T_cur) * kModLen[m] + k] = generated(idx, b, m, k);
            }
            hist[m].swap(nw);
        }
        T_cur += 1;
    }
    return seen;
}

// The driver's form: one sequence [B * N][T_in + new_frames] filled from the caller's B scenes (branch i reads scene i / N), frame f = T_in + idx
// conditioned on cond_window(f, cond) of it, the overwrite in place at frame f - 1, the new frame written at f
static std::vector<TokenSeqs> windows_sequence(const TokenSeqs& in, int B, int N, int T_in, int new_frames, int cond, int ctl_frame) {
    const int BN = B * N, T_out = T_in + new_frames;
    TokenSeqs seq;
    seq.resize(BN, T_out);
    copy_frames(in.view(), BN, [N](size_t i) { return i / N; }, [](size_t) { return 0; }, T_in, seq, 0);
    std::vector<TokenSeqs> seen;
    for (int idx = 0; idx < new_frames; ++idx) {
        const int f = T_in + idx;
        const CondWindow w = cond_window(f, cond);
        if (idx == ctl_frame)
            for (int i = 0; i < BN; ++i)
                for (int k = 0; k < kModLen[2]; k += 7) seq.at(2, i, f - 1)[k] = control_box(i, k);
        TokenSeqs win;
        gather_windows(seq.view(), BN, w.start, w.n, win);
        seen.push_back(win);
        for (int m = 0; m < 4; ++m)
            for (int i = 0; i < BN; ++i)
                for (int k = 0; k < kModLen[m]; ++k) seq.at(m, i, f)[k] = generated(idx, i, m, k);
    }
    return seen;
}

static void test_driver_windows() {
    const int B = 2, N = 3;
    for (int T_in = 1; T_in <= 3; ++T_in)
        for (int nf = 0; nf <= 4; ++nf)
            for (int cond = 1; cond <= 3; ++cond) {
                const TokenSeqs in = make_seqs(B, T_in);
                // the fan form against the gather over an explicitly replicated input
                TokenSeqs rep, fan, flat;
                rep.resize((size_t)B * N, T_in);
                for (int m = 0; m < 4; ++m)
                    for (int b = 0; b < B; ++b)
                        for (int s = 0; s < N; ++s)
                            memcpy(rep.at(m, (size_t)b * N + s, 0), in.view().at(m, b, 0), (size_t)T_in * kModLen[m] * sizeof(int));
                const CondWindow w0 = cond_window(T_in, cond);
                gather_fan_windows(in.view(), 0, (size_t)B * N, N, w0.start, w0.n, fan);
                gather_windows(rep.view(), (size_t)B * N, w0.start, w0.n, flat);
                for (int m = 0; m < 4; ++m) CHECK(fan.frames == flat.frames && fan.mod[m] == flat.mod[m], "fan gather T_in %d cond %d modality %d", T_in, cond, m);
                // the overwrite sits at the frame whose successor's window slides when there is one (cond frames already held), else at the first frame
                const int ctl_frame = nf >= 2 && T_in + 1 > cond && cond >= 2 ? 1 : 0;
                const std::vector<TokenSeqs> was = windows_slide_append(rep, B * N, T_in, nf, cond, ctl_frame);
                const std::vector<TokenSeqs> now = windows_sequence(in, B, N, T_in, nf, cond, ctl_frame);
                CHECK(was.size() == (size_t)nf && now.size() == (size_t)nf, "frame count T_in %d nf %d cond %d", T_in, nf, cond);
                for (size_t idx = 0; idx < was.size() && idx < now.size(); ++idx) {
                    CHECK(was[idx].frames == now[idx].frames, "T_in %d nf %d cond %d frame %zu: %d against %d slots", T_in, nf, cond, idx, was[idx].frames, now[idx].frames);
                    for (int m = 0; m < 4; ++m) CHECK(was[idx].mod[m] == now[idx].mod[m], "T_in %d nf %d cond %d frame %zu modality %d", T_in, nf, cond, idx, m);
                }
                // ... and it did survive a slide: the window behind the control frame still holds the control boxes, one slot further back
                if (ctl_frame == 1 && nf >= 3) {
                    const TokenSeqs& next = now[2];
                    CHECK(next.frames == cond, "the window behind the control frame slid");
                    for (int i = 0; i < B * N; ++i) CHECK(next.view().at(2, i, cond - 2)[7] == control_box(i, 7), "overwrite lost, T_in %d nf %d cond %d item %d", T_in, nf, cond, i);
                }
            }
}

int main() {
    test_layout();
    test_cond_window();
    test_gather();
    test_frame_rows_and_narrow();
    test_driver_windows();
    if (g_fail) {
        printf("token_windows_test: %d checks FAILED\n", g_fail);
        return 1;
    }
    printf("token_windows_test: ok\n");
    return 0;
}
