// Host test of umgen_amd/csrc/gen_side.h (started by tests/test_gen_side_host.py; no GPU, no HIP): GenSide::deliver and side_buffers against
// element-by-element indexing.  A call over 3 scenes and new_frames = 2 delivers scene b of frame idx to item b * 2 + idx of the caller's arrays; for
// topk in {0, 1, 5, 16} every member is asked alone, all together, and all together with one modality pointer missing in every group.  The caller's
// arrays start as a sentinel and carry a guard tail; everything deliver must not touch -- other items, arrays not handed over, list entries past
// topk, the tails -- has to keep it.
#include <cstdio>
#include <cstdlib>

#include "gen_side.h"

using namespace umgen;

static int g_fail = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (++g_fail <= 20) { printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                                              \
    } while (0)

constexpr int kScenes = 3, kNewFrames = 2, kItems = kScenes * kNewFrames, kGuard = 64, kSentinel = -7;
enum Group { G_LOGP, G_LOGZ, G_RANK, G_MASS, G_ENT, G_TOK, G_TLP, G_COUNT };
static bool is_int(int g) { return g == G_RANK || g == G_TOK; }
static bool is_list(int g) { return g == G_TOK || g == G_TLP; }

// a value that names its place in a frame buffer: (group, frame, scene, row position, list entry); < 2^24, so exact as a float too
static int code(int g, int idx, int b, int pos, int j) { return ((((g * kNewFrames + idx) * kScenes + b) * kFrameRowLen + pos) * kSideTopK + j) + 1; }

// the caller's arrays of one group: per modality [kItems][S_mod] (lists x topk) plus the guard tail, as ints or floats of the same value
struct Arrays {
    std::vector<int> i[4];
    std::vector<float> f[4];
    void reset(int g, int topk) {
        for (int m = 0; m < 4; ++m) {
            const size_t n = (size_t)kItems * kModLen[m] * (is_list(g) ? (topk ? topk : 1) : 1) + kGuard;
            i[m].assign(is_int(g) ? n : 0, kSentinel);
            f[m].assign(is_int(g) ? 0 : n, (float)kSentinel);
        }
    }
    int at(int g, int m, size_t k) const { return is_int(g) ? i[m][k] : (int)f[m][k]; }
    size_t size(int g, int m) const { return is_int(g) ? i[m].size() : f[m].size(); }
};

struct Request {
    bool ask[G_COUNT];
    int skip_mod;      // this modality's pointer is missing in every group asked for (-1: none)
    bool has(int g, int m) const { return ask[g] && m != skip_mod; }
};

static SideDst make_dst(const Request& rq, Arrays (&a)[G_COUNT], int topk) {
    SideDst d{};
    for (int m = 0; m < 4; ++m) {
        if (rq.has(G_LOGP, m)) d.logp[m] = a[G_LOGP].f[m].data();
        if (rq.has(G_LOGZ, m)) d.logz[m] = a[G_LOGZ].f[m].data();
        if (rq.has(G_RANK, m)) d.rank[m] = a[G_RANK].i[m].data();
        if (rq.has(G_MASS, m)) d.mass_above[m] = a[G_MASS].f[m].data();
        if (rq.has(G_ENT, m)) d.entropy[m] = a[G_ENT].f[m].data();
        if (rq.has(G_TOK, m)) d.topk_tok[m] = a[G_TOK].i[m].data();
        if (rq.has(G_TLP, m)) d.topk_logp[m] = a[G_TLP].f[m].data();
    }
    d.topk = topk;
    return d;
}

// the frame buffers of frame idx, every entry of every buffer the call formed (the list entries past topk too: they must stay where they are)
static void fill_frame(GenSide& gs, int idx) {
    std::vector<float>* const fb[G_COUNT] = {&gs.f_logp, &gs.f_logz, nullptr, &gs.f_mass, &gs.f_ent, nullptr, &gs.f_tlp};
    std::vector<int>* const ib[G_COUNT] = {nullptr, nullptr, &gs.f_rank, nullptr, nullptr, &gs.f_tok, nullptr};
    for (int g = 0; g < G_COUNT; ++g) {
        const size_t per = is_list(g) ? kSideTopK : 1, n = is_int(g) ? ib[g]->size() : fb[g]->size();
        CHECK(n == 0 || n == (size_t)kScenes * kFrameRowLen * per, "group %d: %zu entries", g, n);
        for (size_t k = 0; k < n; ++k) {
            const int v = code(g, idx, (int)(k / per / kFrameRowLen), (int)(k / per % kFrameRowLen), (int)(k % per));
            if (is_int(g)) (*ib[g])[k] = v; else (*fb[g])[k] = (float)v;
        }
    }
}

// every element of every array: what the deliveries so far (delivered[item]: the frame that went there, or -1) must have left
static void check_arrays(const Request& rq, const Arrays (&a)[G_COUNT], int topk, const int (&delivered)[kItems], const char* what) {
    for (int g = 0; g < G_COUNT; ++g)
        for (int m = 0; m < 4; ++m) {
            const size_t per = is_list(g) ? (size_t)(topk ? topk : 1) : 1, body = (size_t)kItems * kModLen[m] * per;
            const bool written = rq.has(g, m) && !(is_list(g) && topk == 0);
            for (size_t k = 0; k < a[g].size(g, m); ++k) {
                int want = kSentinel;
                const size_t item = k / per / kModLen[m];
                if (written && k < body && delivered[item] >= 0)
                    want = code(g, delivered[item], (int)(item / kNewFrames), kModOff[m] + (int)(k / per % kModLen[m]), (int)(k % per));
                if (a[g].at(g, m, k) != want) { CHECK(false, "%s: topk %d group %d modality %d element %zu is %d, not %d", what, topk, g, m, k, a[g].at(g, m, k), want); return; }
            }
        }
}

// the device bundle as side_buffers reads it (TokenSide's member names, frame.h), with addresses that are never followed
struct FakeDetail { int* rank; float *mass_above, *entropy; int* topk_tok; float* topk_logp; };
struct FakeSide { float *logp, *logz; FakeDetail detail; };

static void check_side_buffers(const Request& rq, const GenSide& gs, int topk) {
    static float fl[5];
    static int in[2];
    const FakeSide dev{&fl[0], &fl[1], FakeDetail{&in[0], &fl[2], &fl[3], &in[1], &fl[4]}};
    bool any = false, detail = false, lists = false;
    for (int g = 0; g < G_COUNT; ++g) {      // (a missing modality leaves three others: the group is still asked for)
        any = any || rq.ask[g];
        detail = detail || (rq.ask[g] && g >= G_RANK);
        lists = lists || (rq.ask[g] && is_list(g));
    }
    lists = lists && topk > 0;
    const FrameSide* h = gs.frame();
    CHECK((h != nullptr) == any, "frame() is %s", h ? "set" : "null");
    if (!h) return;
    CHECK(h->topk == (lists ? topk : 0), "topk %d of %d", h->topk, topk);
    for (size_t B : {(size_t)1, (size_t)kScenes}) {
        const size_t row = B * kFrameRowLen * 4;
        SideBuf want[7];
        int n = 0;
        if (rq.ask[G_LOGP]) want[n++] = SideBuf{dev.logp, gs.fs.logp, row};
        if (rq.ask[G_LOGZ]) want[n++] = SideBuf{dev.logz, gs.fs.logz, row};
        if (detail) {
            want[n++] = SideBuf{dev.detail.rank, gs.fs.rank, row};
            want[n++] = SideBuf{dev.detail.mass_above, gs.fs.mass_above, row};
            want[n++] = SideBuf{dev.detail.entropy, gs.fs.entropy, row};
            if (lists) {
                want[n++] = SideBuf{dev.detail.topk_tok, gs.fs.topk_tok, row * kSideTopK};
                want[n++] = SideBuf{dev.detail.topk_logp, gs.fs.topk_logp, row * kSideTopK};
            }
        }
        const SideBufs got = side_buffers(dev, *h, B);
        CHECK(got.n == n && got.end() - got.begin() == n, "%d buffers listed, %d expected", got.n, n);
        for (int k = 0; k < n && k < got.n; ++k)
            CHECK(got.buf[k].dev == want[k].dev && got.buf[k].host == want[k].host && want[k].host != nullptr && got.buf[k].bytes == want[k].bytes,
                  "buffer %d of %d: %zu bytes, %zu expected", k, n, got.buf[k].bytes, want[k].bytes);
    }
    // the host pointers are the owner's own buffers, sized for the call's scenes
    const size_t n = (size_t)kScenes * kFrameRowLen;
    CHECK(gs.f_logp.size() == (rq.ask[G_LOGP] ? n : 0) && gs.f_logz.size() == (rq.ask[G_LOGZ] ? n : 0), "logp %zu logz %zu", gs.f_logp.size(), gs.f_logz.size());
    CHECK(gs.f_rank.size() == (detail ? n : 0) && gs.f_mass.size() == gs.f_rank.size() && gs.f_ent.size() == gs.f_rank.size(), "detail %zu", gs.f_rank.size());
    CHECK(gs.f_tok.size() == (lists ? n * kSideTopK : 0) && gs.f_tlp.size() == gs.f_tok.size(), "lists %zu", gs.f_tok.size());
    CHECK(h->logp == (gs.f_logp.empty() ? nullptr : gs.f_logp.data()) && h->rank == (gs.f_rank.empty() ? nullptr : gs.f_rank.data()) &&
              h->topk_logp == (gs.f_tlp.empty() ? nullptr : gs.f_tlp.data()), "frame() points at the owner's buffers");
}

static void run_request(const Request& rq, int topk, bool check_every_delivery, const char* what) {
    static Arrays a[G_COUNT];
    for (int g = 0; g < G_COUNT; ++g) a[g].reset(g, topk);
    GenSide gs;
    gs.init(make_dst(rq, a, topk), kScenes);
    check_side_buffers(rq, gs, topk);
    int delivered[kItems];
    for (int& d : delivered) d = -1;
    for (int idx = 0; idx < kNewFrames; ++idx) {
        fill_frame(gs, idx);
        for (int b = 0; b < kScenes; ++b) {
            gs.deliver((size_t)b, (size_t)b * kNewFrames + idx);
            delivered[b * kNewFrames + idx] = idx;
            if (check_every_delivery) check_arrays(rq, a, topk, delivered, what);
        }
    }
    check_arrays(rq, a, topk, delivered, what);
}

int main() {
    const char* const names[G_COUNT] = {"logp", "logz", "rank", "mass_above", "entropy", "topk_tok", "topk_logp"};
    for (int topk : {0, 1, 5, 16}) {
        for (int g = 0; g < G_COUNT; ++g) {      // every member alone
            Request rq{{}, -1};
            rq.ask[g] = true;
            run_request(rq, topk, false, names[g]);
        }
        Request all{{true, true, true, true, true, true, true}, -1};
        run_request(all, topk, true, "all");
        for (int m = 0; m < 4; ++m) {            // ... and a modality pointer missing inside every group
            all.skip_mod = m;
            run_request(all, topk, false, "all but one modality");
        }
        run_request(Request{{}, -1}, topk, false, "nothing");
    }
    if (g_fail) { printf("gen_side_test: %d check(s) failed\n", g_fail); return 1; }
    printf("gen_side_test: ok\n");
    return 0;
}
