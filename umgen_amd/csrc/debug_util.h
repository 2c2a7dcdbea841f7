// What the kernel-level test hooks (debug_gemm_attn.hip, debug_decode.hip, debug_frame.hip) share: the device scratch of one hook call with
// its guard bands, fills, the precision dispatch and the timing loop.  Internal to those files; never part of the product path.
//
// A hook body reads: validate, sizes, buffers (Scratch), one `if (s.rc) return s.rc;`, fills, launch through the product's launcher,
// s.finish() (launch errors, the work, every guard band), downloads.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/umgen.h"
#include "frame.h"
#include "kernels.h"

using namespace umgen;

namespace {
inline int up(void* d, const void* h, size_t n) { return hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : UMGEN_E_HIP; }
inline int down(void* h, const void* d, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : UMGEN_E_HIP; }

// Guard band: the sentinel bytes behind an output buffer.  A kernel that writes past N, M or the row changes the band; the hook then
// returns UMGEN_E_STATE.
constexpr unsigned char kGuardByte = 0xA7;
constexpr size_t kGuardBytes = (size_t)64 << 10;

// launch errors first (a launch the runtime refused writes nothing), then the work itself
inline int finish() {
    if (hipGetLastError() != hipSuccess) return UMGEN_E_HIP;
    return hipDeviceSynchronize() == hipSuccess ? UMGEN_OK : UMGEN_E_HIP;
}

// a device pointer of Scratch, taken as whatever pointer type the launcher wants
struct DevPtr {
    void* p = nullptr;
    template <typename T> operator T*() const { return (T*)p; }
};

// Every device buffer of ONE hook call; frees them all at scope exit.  The first failure sticks in rc.
struct Scratch {
    int rc = UMGEN_OK;                 // UMGEN_E_NOMEM (allocation) or UMGEN_E_HIP (copy / fill)
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    ~Scratch() { for (void* p : bufs) (void)hipFree(p); }
    // uninitialised
    DevPtr raw(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { fail(UMGEN_E_NOMEM); return {}; }
        bufs.push_back(p);
        return {p};
    }
    // allocate + upload; a nullable operand (ln_w, bias, forced, ...) that is absent stays nullptr on the device side too
    DevPtr in(const void* host, size_t bytes) {
        if (!host) return {};
        DevPtr d = raw(bytes);
        if (d.p && up(d.p, host, bytes)) fail(UMGEN_E_HIP);
        return d;
    }
    // `bytes` the kernel may write, then a band of `band` sentinel bytes that intact() checks
    DevPtr out(size_t bytes, size_t band = kGuardBytes) {
        DevPtr d = raw(bytes + band);
        if (!d.p) return d;
        if (hipMemset((char*)d.p + bytes, kGuardByte, band) != hipSuccess) fail(UMGEN_E_HIP);
        bands.push_back({(const char*)d.p + bytes, band});
        return d;
    }
    // out() for an in / out argument: starts as the caller's buffer
    DevPtr inout(const void* host, size_t bytes, size_t band = kGuardBytes) {
        DevPtr d = out(bytes, band);
        if (d.p && bytes && up(d.p, host, bytes)) fail(UMGEN_E_HIP);
        return d;
    }
    // every band of every out() buffer still holds the sentinel
    bool intact() const {
        for (const auto& b : bands) {
            std::vector<unsigned char> h(b.second);
            if (down(h.data(), b.first, h.size())) return false;
            for (unsigned char c : h)
                if (c != kGuardByte) return false;
        }
        return true;
    }
    // what follows the launches: finish(), then the bands (UMGEN_E_STATE)
    int finish() const {
        if (int r = ::finish()) return r;
        return intact() ? UMGEN_OK : UMGEN_E_STATE;
    }

private:
    std::vector<void*> bufs;
    std::vector<std::pair<const char*, size_t>> bands;
    void fail(int code) { if (!rc) rc = code; }
};

// band behind a buffer of M per-scene rows: the rows scenes M .. kRowsMaxM - 1 would take (at least 64 KB, at most 64 MB)
inline size_t scene_band(size_t row_bytes, int M) {
    return std::min(std::max(kGuardBytes, row_bytes * (size_t)(kRowsMaxM - M)), (size_t)64 << 20);
}

constexpr unsigned kNaN32 = 0x7fc00000u;
constexpr float kStalePartial = 1000.f;   // never-written slots of the attention partials: finite garbage, like the product's stale values
inline unsigned short nan16(int prec) { return prec == 2 ? 0x7e00 : 0x7fc0; }
// n 32-bit words of one pattern (the NaN of fp32 buffers, kStalePartial)
inline int fill_words(void* d, unsigned word, size_t n) { return hipMemsetD32((hipDeviceptr_t)d, (int)word, n) == hipSuccess ? 0 : UMGEN_E_HIP; }
inline int fill_stale(void* d, size_t n) { return fill_words(d, __builtin_bit_cast(unsigned, kStalePartial), n); }
// n elements of the quiet NaN of precision code prec (0 fp32, 1 bf16, 2 fp16): a location the kernel leaves out comes back as NaN
inline int fill_nan(void* d, size_t n, int prec) {
    if (!prec) return fill_words(d, kNaN32, n);
    return hipMemsetD16((hipDeviceptr_t)d, nan16(prec), n) == hipSuccess ? 0 : UMGEN_E_HIP;
}

// floats of a fragment-major buffer of kRowsMaxM scenes x C columns (frag_index, kernels.h)
inline size_t frag_floats(int C) { return (size_t)((C + 31) / 32) * 32 * kRowsMaxM; }
// fragment-major [kRowsMaxM][C] on the device -> row-major [M][C] on the host; UMGEN_E_STATE if a column m >= M or a pad column >= C was written
inline int frag_down(const void* d, int M, int C, float* rows) {
    std::vector<unsigned> h(frag_floats(C));
    if (int rc = down(h.data(), d, h.size() * 4)) return rc;
    bool clean = true;
    for (int m = 0; m < kRowsMaxM; ++m)
        for (int c = 0; c < (C + 31) / 32 * 32; ++c) {
            const unsigned v = h[frag_index(m, c)];
            if (m < M && c < C) memcpy(rows + (size_t)m * C + c, &v, 4);
            else clean = clean && v == kNaN32;
        }
    return clean ? UMGEN_OK : UMGEN_E_STATE;
}

// f(T{}) with T the operand type of precision code prec (0 fp32, 1 bf16, 2 fp16)
template <typename F>
void by_prec(int prec, F&& f) {
    if (prec == 2) f(f16_t{}); else if (prec == 1) f(bf16_t{}); else f(float{});
}
// the same for the hooks that exist only for the 16-bit types (1 bf16, 2 fp16)
template <typename F>
void by_prec16(int prec, F&& f) {
    if (prec == 2) f(f16_t{}); else f(bf16_t{});
}

inline bool in_range(const int32_t* t, size_t n, int hi) {
    for (size_t i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= hi) return false;
    return true;
}
inline int kind_of_pos(int j, int given_end) {    // the decode loops' step_kind (engine_frame.hip): 0 fixed token, 1 map, 2 bbox3d, 3 image
    if (j < given_end) return 0;
    return (j >= kMapC0 && j < kMapEos) ? 1 : (j >= kBoxC0 && j < kBoxEos) ? 2 : (j >= kImgC0 && j < kImgEos) ? 3 : 0;
}

// ---- timing hooks ----
// n bf16 values in [-scale, scale) from the linear congruential sequence x (continued across calls)
inline void fill_lcg(std::vector<bf16_t>& h, size_t n, unsigned& x, float scale) {
    h.resize(n);
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = f32_to_bf16((((x >> 8) & 0xffff) / 32768.0f - 1.0f) * scale); }
}
struct Stream {
    hipStream_t s = nullptr;
    Stream() { if (hipStreamCreate(&s) != hipSuccess) s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    Stream(const Stream&) = delete;
};
// n_series measurements on one event pair: `warm` untimed calls of fn(i), then `iters` calls between two events on `stream`;
// ms_each[i] = the average milliseconds per call of series i
template <typename F>
int time_launches(hipStream_t stream, int warm, int iters, int n_series, float* ms_each, F&& fn) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (hipEventCreate(&ev.e0) != hipSuccess || hipEventCreate(&ev.e1) != hipSuccess) return UMGEN_E_HIP;
    for (int i = 0; i < n_series; ++i) {
        for (int k = 0; k < warm; ++k) fn(i);
        (void)hipEventRecord(ev.e0, stream);
        for (int k = 0; k < iters; ++k) fn(i);
        (void)hipEventRecord(ev.e1, stream);
        if (hipGetLastError() != hipSuccess || hipEventSynchronize(ev.e1) != hipSuccess) return UMGEN_E_HIP;
        float t = 0.f;
        (void)hipEventElapsedTime(&t, ev.e0, ev.e1);
        ms_each[i] = t / (float)iters;
    }
    return UMGEN_OK;
}
}  // namespace
