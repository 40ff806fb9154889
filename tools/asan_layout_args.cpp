// Stand-alone host check of the capacity-layout entry points (include/dsp_frontend.h: dsp_frames_bound, dsp_batch_offsets_batch,
// dsp_layout_create_capacity, dsp_layout_refresh; csrc/dsp_frontend.hip).  Every argument error is DSP_EINVAL with a message
// before any device call, the bound is checked at its overflow edge, and under dsp_debug_host_dry_run(1) what passed every check is
// refused instead of launched (a capacity handle made there keeps its tables in host memory and can only be destroyed): the
// program needs no GPU.  `make -C dsp-speech-recognition_amd/csrc asan-layout` builds it with AddressSanitizer + UBSan against
// the sanitized build of the library and runs it; it needs no preloaded runtime.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "asan_args.h"
#include "dsp_frontend.h"

static void expect_bound(int64_t cap, int32_t n, int32_t L, int32_t S, int64_t want, int line) {
    int64_t got = -1;
    const int rc = dsp_frames_bound(cap, n, L, S, &got);
    if (rc != DSP_OK || got != want) {
        std::printf("line %d: dsp_frames_bound rc %d, %lld, expected %lld\n", line, rc, (long long)got, (long long)want);
        ++g_bad;
    }
}
#define BOUND(cap, n, L, S, want) expect_bound((cap), (n), (L), (S), (want), __LINE__)

int main() {
    dsp_debug_host_dry_run(1);
    const char* refused = "dry_run: launches are refused";
    // never reached by a kernel: every call below returns before a launch
    static int64_t in[8] = {0, 10, 20, 30}, out[8], fo0[8], fo1[8], fo2[8], fo3[8];
    static int32_t status[1];
    const int32_t L[5] = {480, 400, 64, 1, 1}, S[5] = {160, 160, 16, 1, 1}, zeroL[2] = {480, 0}, negS[2] = {-1, 160};
    int64_t* const tabs[5] = {fo0, fo1, fo2, fo3, fo3};
    int64_t* const with_null[2] = {fo0, nullptr};
    int64_t* const shared[2] = {fo0, fo0};
    int64_t* const on_out[2] = {out, fo1};
    int64_t* const on_in[2] = {fo0, in};
    const int64_t i64max = INT64_MAX;
    int64_t b = 0;

    // ---- dsp_frames_bound: checks, values, the overflow edge ----
    EXPECT(dsp_frames_bound(1000, 3, 480, 160, nullptr), "n_frames_bound is NULL");
    EXPECT(dsp_frames_bound(-1, 3, 480, 160, &b), "sample_capacity >= 0");
    EXPECT(dsp_frames_bound(1000, 0, 480, 160, &b), "n_utt > 0");
    EXPECT(dsp_frames_bound(1000, -4, 480, 160, &b), "n_utt > 0");
    EXPECT(dsp_frames_bound(1000, 3, 0, 160, &b), "frame_len > 0");
    EXPECT(dsp_frames_bound(1000, 3, 480, 0, &b), "frame_step > 0");
    BOUND(0, 3, 480, 160, 3);
    BOUND(1000, 3, 480, 160, 6 + 3);                 // L >= S: one frame per clip on top
    BOUND(1000, 3, 160, 480, 2 + 6);                 // L < S: two
    BOUND(i64max - 1, 1, 480, 1, i64max);            // the last capacity that fits at a hop of one sample
    EXPECT(dsp_frames_bound(i64max, 1, 480, 1, &b), "overflows int64");
    EXPECT(dsp_frames_bound(i64max, 1, 1, 1, &b), "overflows int64");
    EXPECT(dsp_frames_bound(i64max, 0x7fffffff, 480, 1, &b), "overflows int64");
    BOUND(i64max, 1, 1, 2, i64max / 2 + 2);          // a longer hop leaves room
    BOUND(i64max - 0x7fffffffLL, 0x7fffffff, 1, 1, i64max);          // the last capacity that fits at the largest n_utt
    EXPECT(dsp_frames_bound(i64max - 0x7fffffffLL + 1, 0x7fffffff, 1, 1, &b), "overflows int64");
    BOUND(i64max - 2 * 0x7fffffffLL, 0x7fffffff, 1, 2, (i64max - 2 * 0x7fffffffLL) / 2 + 2 * 0x7fffffffLL);

    // ---- dsp_batch_offsets_batch ----
    EXPECT(dsp_batch_offsets_batch(nullptr, 3, 1000, 2, L, S, out, tabs, status, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, nullptr, tabs, status, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, tabs, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, nullptr, S, out, tabs, status, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, nullptr, out, tabs, status, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, nullptr, status, nullptr), "NULL argument");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, with_null, status, nullptr), "framing 1: NULL frame offsets");
    EXPECT(dsp_batch_offsets_batch(in, 0, 1000, 2, L, S, out, tabs, status, nullptr), "n_utt 0 must be >= 1");
    EXPECT(dsp_batch_offsets_batch(in, -2, 1000, 2, L, S, out, tabs, status, nullptr), "n_utt -2 must be >= 1");
    EXPECT(dsp_batch_offsets_batch(in, 3, 0, 2, L, S, out, tabs, status, nullptr), "sample_capacity 0 must be >= 1");
    EXPECT(dsp_batch_offsets_batch(in, 3, -1000, 2, L, S, out, tabs, status, nullptr), "sample_capacity -1000 must be >= 1");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 5, L, S, out, tabs, status, nullptr), "n_framings 5 must be in [0, 4]");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, -1, L, S, out, tabs, status, nullptr), "n_framings -1 must be in [0, 4]");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, zeroL, S, out, tabs, status, nullptr), "framing 1: frame_len 0");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, negS, out, tabs, status, nullptr), "framing 0: frame_len 480 and frame_step -1");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, in, tabs, status, nullptr), "overlap");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, shared, status, nullptr), "overlap");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, on_out, status, nullptr), "overlap");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, on_in, status, nullptr), "overlap");
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 2, L, S, out, tabs, status, nullptr), refused);
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 4, L, S, out, tabs, status, nullptr), refused);          // the most framings
    EXPECT(dsp_batch_offsets_batch(in, 3, 1000, 0, nullptr, nullptr, out, nullptr, status, nullptr), refused);   // none
    EXPECT(dsp_batch_offsets_batch(in, 0x7fffffff, i64max, 1, L, S, out, tabs, status, nullptr), refused);

    // ---- dsp_layout_create_capacity / dsp_layout_refresh / a launch on the handle ----
    dsp_layout* h = nullptr;
    EXPECT(dsp_layout_create_capacity(3, 100, 480, 160, nullptr), "out is NULL");
    EXPECT(dsp_layout_create_capacity(0, 100, 480, 160, &h), "need n_utt > 0");
    EXPECT(dsp_layout_create_capacity(3, 0, 480, 160, &h), "need n_utt > 0");
    EXPECT(dsp_layout_create_capacity(3, -5, 480, 160, &h), "need n_utt > 0");
    EXPECT(dsp_layout_create_capacity(3, 100, 0, 160, &h), "need n_utt > 0");
    EXPECT(dsp_layout_create_capacity(3, 100, 480, 0, &h), "need n_utt > 0");
    EXPECT(dsp_layout_create_capacity(5, 4, 480, 160, &h), "below one frame per clip");
    EXPECT(dsp_layout_create_capacity(1, (int64_t)1 << 40, 480, 160, &h), "batch too large");
    EXPECT(dsp_layout_create_capacity(1, i64max, 1323, 441, &h), "batch too large");
    if (h != nullptr) { std::printf("a refused create left a handle\n"); ++g_bad; }
    const int32_t framings[3][2] = {{480, 160}, {1323, 441}, {48, 16}};     // 16-frame groups; 4- and 8-frame groups; no tables
    for (const auto& f : framings) {
        h = nullptr;
        if (dsp_layout_create_capacity(7, 1000, f[0], f[1], &h) != DSP_OK || h == nullptr) {
            std::printf("dsp_layout_create_capacity(%d, %d) failed: %s\n", f[0], f[1], dsp_last_error());
            ++g_bad;
            continue;
        }
        static double amp[4];
        static int16_t wave[16];
        EXPECT(dsp_layout_refresh(nullptr, fo0, nullptr), "NULL argument");
        EXPECT(dsp_layout_refresh(h, nullptr, nullptr), "NULL argument");
        EXPECT(dsp_layout_refresh(h, fo0, nullptr), refused);
        EXPECT(dsp_vad_features_layout_batch(h, wave, DSP_WAVE_I16, out, fo0, 0, amp, status, nullptr), refused);
        if (dsp_layout_destroy(h) != DSP_OK) { std::printf("dsp_layout_destroy failed\n"); ++g_bad; }
    }

    dsp_debug_host_dry_run(0);
    return finish("asan_layout_args");
}
