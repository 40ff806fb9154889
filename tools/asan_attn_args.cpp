// Stand-alone host check of the attention entry points (include/dsp_frontend.h: dsp_attn_create, dsp_attn_destroy,
// dsp_attn_workspace_bytes, dsp_attn_forward, dsp_selfattn_pool_batch, and the training ones: dsp_attn_tape_bytes,
// dsp_attn_forward_train, dsp_attn_backward_bytes, dsp_attn_backward, dsp_selfattn_pool_train_batch,
// dsp_selfattn_pool_backward_batch; csrc/dsp_attn.hip).  Create packs the backward's six matrices with the forward's.  Under dsp_debug_host_dry_run(1)
// create reads its parameters as host memory and packs them there, so the packing runs here -- on exact-size arrays, where a
// read past either end of a parameter is a report -- and every argument error is DSP_EINVAL with a message before any device
// call: the program needs no GPU.  `make -C dsp-speech-recognition_amd/csrc asan-attn` builds it with AddressSanitizer + UBSan
// against the sanitized build of the library and runs it; it needs no preloaded runtime.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "asan_args.h"
#include "dsp_frontend.h"

// The 13 parameters of a block as exact-size host arrays.
struct Block {
    std::vector<std::vector<float>> p;
    dsp_attn_desc d;
    Block(int dm, int di, int dk, int dv) {
        const size_t n[DSP_ATTN_PARAMS] = {(size_t)dm * dk, (size_t)dm * dk, (size_t)dm * dv, (size_t)dm, (size_t)dm, (size_t)dm * dv, (size_t)dm,
                                           (size_t)di * dm, (size_t)di, (size_t)dm * di, (size_t)dm, (size_t)dm, (size_t)dm};
        d = dsp_attn_desc{dm, di, 1, dk, dv, 1e-3f, {}};
        for (int i = 0; i < DSP_ATTN_PARAMS; ++i) {
            p.emplace_back(n[i]);
            for (size_t j = 0; j < n[i]; ++j) p[i][j] = 0.001f * (float)((j * 7 + i) % 311) - 0.1f;
            d.d_params[i] = p[i].data();
        }
    }
};

int main() {
    dsp_debug_host_dry_run(1);
    const int sizes[][4] = {{39, 200, 100, 100}, {6, 8, 4, 12}, {1, 4, 4, 4}, {64, 256, 128, 128}, {17, 36, 20, 52}};
    dsp_attn* keep = nullptr;
    for (const auto& s : sizes) {
        Block blk(s[0], s[1], s[2], s[3]);
        dsp_attn* h = nullptr;
        EXPECT_OK(dsp_attn_create(&blk.d, &h));
        if (h && !keep) { keep = h; continue; }
        EXPECT_OK(dsp_attn_destroy(h));
    }
    EXPECT_OK(dsp_attn_destroy(nullptr));

    Block good(39, 200, 100, 100);
    dsp_attn* h = nullptr;
    EXPECT(dsp_attn_create(nullptr, &h), "NULL argument");
    EXPECT(dsp_attn_create(&good.d, nullptr), "NULL argument");
    { dsp_attn_desc d = good.d; d.n_head = 2; EXPECT(dsp_attn_create(&d, &h), "n_head 2 must be 1"); }
    { dsp_attn_desc d = good.d; d.d_model = 0; EXPECT(dsp_attn_create(&d, &h), "d_model 0 must be in [1, 64]"); }
    { dsp_attn_desc d = good.d; d.d_model = 65; EXPECT(dsp_attn_create(&d, &h), "d_model 65 must be in [1, 64]"); }
    { dsp_attn_desc d = good.d; d.d_k = 102; EXPECT(dsp_attn_create(&d, &h), "must be multiples of 4 in [4, 128]"); }
    { dsp_attn_desc d = good.d; d.d_k = 0; EXPECT(dsp_attn_create(&d, &h), "must be multiples of 4 in [4, 128]"); }
    { dsp_attn_desc d = good.d; d.d_v = 132; EXPECT(dsp_attn_create(&d, &h), "must be multiples of 4 in [4, 128]"); }
    { dsp_attn_desc d = good.d; d.d_inner = 260; EXPECT(dsp_attn_create(&d, &h), "d_inner 260 must be a multiple of 4 in [4, 256]"); }
    { dsp_attn_desc d = good.d; d.d_inner = 201; EXPECT(dsp_attn_create(&d, &h), "d_inner 201 must be a multiple of 4 in [4, 256]"); }
    { dsp_attn_desc d = good.d; d.eps = std::numeric_limits<float>::quiet_NaN(); EXPECT(dsp_attn_create(&d, &h), "eps must be finite"); }
    { dsp_attn_desc d = good.d; d.eps = -1.f; EXPECT(dsp_attn_create(&d, &h), "eps must be finite"); }
    for (int i = 0; i < DSP_ATTN_PARAMS; ++i) {
        dsp_attn_desc d = good.d;
        d.d_params[i] = nullptr;
        EXPECT(dsp_attn_create(&d, &h), "NULL parameter tensor");
    }

    if (keep) {
        int64_t bytes = 0;
        EXPECT(dsp_attn_workspace_bytes(nullptr, 200, 8, &bytes), "NULL argument");
        EXPECT(dsp_attn_workspace_bytes(keep, 200, 8, nullptr), "NULL argument");
        EXPECT(dsp_attn_workspace_bytes(keep, 0, 8, &bytes), "T 0 must be in [1, 1024]");
        EXPECT(dsp_attn_workspace_bytes(keep, 1025, 8, &bytes), "T 1025 must be in [1, 1024]");
        EXPECT(dsp_attn_workspace_bytes(keep, 200, 0, &bytes), "B 0 must be >= 1");
        EXPECT(dsp_attn_workspace_bytes(keep, 1024, 0x7fffffff, &bytes), "more than one launch holds");
        EXPECT_OK(dsp_attn_workspace_bytes(keep, 200, 512, &bytes));
        if (bytes <= 0 || bytes >= (int64_t)4 * 512 * 200 * 200) { std::printf("workspace at (200, 512): %lld bytes\n", (long long)bytes); ++g_bad; }
        EXPECT_OK(dsp_attn_workspace_bytes(keep, 5, 3, &bytes));
        alignas(16) static float x[5 * 3 * 39], y[5 * 3 * 39], work[16];   // never reached: every call below returns before a launch
        EXPECT(dsp_attn_forward(nullptr, x, 5, 3, y, work, bytes, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward(keep, nullptr, 5, 3, y, work, bytes, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward(keep, x, 5, 3, nullptr, work, bytes, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward(keep, x, 0, 3, y, work, bytes, nullptr), "T 0 must be in [1, 1024]");
        EXPECT(dsp_attn_forward(keep, x, 5, -1, y, work, bytes, nullptr), "B -1 must be >= 1");
        EXPECT(dsp_attn_forward(keep, x, 5, 3, y, nullptr, bytes, nullptr), "the workspace holds 0 bytes");
        EXPECT(dsp_attn_forward(keep, x, 5, 3, y, work, bytes - 1, nullptr), "are needed");
        EXPECT(dsp_attn_forward(keep, x, 5, 3, y, reinterpret_cast<char*>(work) + 4, bytes, nullptr), "d_work must be 16-byte aligned");
        EXPECT(dsp_attn_forward(keep, x, 5, 3, y, work, bytes, nullptr), "dry_run: launches are refused");

        // ---- training: tape / work / da byte counts and the checks of forward_train and backward
        int64_t tape = 0, wk = 0, da = 0;
        EXPECT(dsp_attn_tape_bytes(nullptr, 200, 8, &tape), "NULL argument");
        EXPECT(dsp_attn_tape_bytes(keep, 200, 8, nullptr), "NULL argument");
        EXPECT(dsp_attn_tape_bytes(keep, 0, 8, &tape), "T 0 must be in [1, 1024]");
        EXPECT(dsp_attn_tape_bytes(keep, 200, 0, &tape), "B 0 must be >= 1");
        EXPECT(dsp_attn_backward_bytes(nullptr, 200, 8, &wk, &da), "NULL argument");
        EXPECT(dsp_attn_backward_bytes(keep, 200, 8, nullptr, &da), "NULL argument");
        EXPECT(dsp_attn_backward_bytes(keep, 200, 8, &wk, nullptr), "NULL argument");
        EXPECT(dsp_attn_backward_bytes(keep, 1025, 8, &wk, &da), "T 1025 must be in [1, 1024]");
        EXPECT(dsp_attn_backward_bytes(keep, 1024, 0x7fffffff, &wk, &da), "more than one launch holds");
        EXPECT_OK(dsp_attn_tape_bytes(keep, 200, 512, &tape));
        EXPECT_OK(dsp_attn_backward_bytes(keep, 200, 512, &wk, &da));
        const int64_t one_btt = (int64_t)4 * 512 * 200 * 200, TP = 208, DP = 48;
        if (tape != 4 * (3 * 512 * TP * DP + 2 * TP * TP) || tape >= one_btt) { std::printf("tape at (200, 512): %lld bytes\n", (long long)tape); ++g_bad; }
        if (wk != 4 * (2 * 512 * TP * DP + TP * TP) || wk >= one_btt) { std::printf("work at (200, 512): %lld bytes\n", (long long)wk); ++g_bad; }
        if (da != (int64_t)4 * 200 * 512 * (4 * 39 + 200 + 100 + 100)) { std::printf("da at (200, 512): %lld bytes\n", (long long)da); ++g_bad; }
        EXPECT_OK(dsp_attn_tape_bytes(keep, 5, 3, &tape));
        EXPECT_OK(dsp_attn_backward_bytes(keep, 5, 3, &wk, &da));
        alignas(16) static float buf[16];                                    // never reached, as above
        char* mis = reinterpret_cast<char*>(buf) + 4;
        EXPECT(dsp_attn_forward_train(nullptr, x, 5, 3, y, buf, tape, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward_train(keep, nullptr, 5, 3, y, buf, tape, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 3, nullptr, buf, tape, nullptr), "NULL handle / input / output");
        EXPECT(dsp_attn_forward_train(keep, x, 0, 3, y, buf, tape, nullptr), "T 0 must be in [1, 1024]");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 0, y, buf, tape, nullptr), "B 0 must be >= 1");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 3, y, nullptr, tape, nullptr), "d_tape holds 0 bytes");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 3, y, buf, tape - 1, nullptr), "are needed");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 3, y, mis, tape, nullptr), "d_tape must be 16-byte aligned");
        EXPECT(dsp_attn_forward_train(keep, x, 5, 3, y, buf, tape, nullptr), "dry_run: launches are refused");
        EXPECT(dsp_attn_backward(nullptr, 5, 3, buf, tape, x, y, buf, da, buf, wk, nullptr), "NULL handle / gradient");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, nullptr, y, buf, da, buf, wk, nullptr), "NULL handle / gradient");
        EXPECT(dsp_attn_backward(keep, 1025, 3, buf, tape, x, y, buf, da, buf, wk, nullptr), "T 1025 must be in [1, 1024]");
        EXPECT(dsp_attn_backward(keep, 5, -1, buf, tape, x, y, buf, da, buf, wk, nullptr), "B -1 must be >= 1");
        EXPECT(dsp_attn_backward(keep, 5, 3, nullptr, tape, x, y, buf, da, buf, wk, nullptr), "d_tape holds 0 bytes");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape - 1, x, y, buf, da, buf, wk, nullptr), "are needed");
        EXPECT(dsp_attn_backward(keep, 5, 3, mis, tape, x, y, buf, da, buf, wk, nullptr), "d_tape must be 16-byte aligned");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, buf, da, nullptr, wk, nullptr), "d_work holds 0 bytes");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, buf, da, buf, wk - 1, nullptr), "are needed");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, buf, da, mis, wk, nullptr), "d_work must be 16-byte aligned");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, nullptr, da, buf, wk, nullptr), "d_da holds 0 bytes");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, buf, da - 1, buf, wk, nullptr), "are needed");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, y, buf, da, buf, wk, nullptr), "dry_run: launches are refused");
        EXPECT(dsp_attn_backward(keep, 5, 3, buf, tape, x, nullptr, buf, da, buf, wk, nullptr), "dry_run: launches are refused");   // d_gx is optional

        // ---- refresh: the descriptor's sizes must be the handle's, no NULL, and a dry-run handle is refused
        EXPECT(dsp_attn_refresh(nullptr, &good.d, nullptr), "NULL argument");
        EXPECT(dsp_attn_refresh(keep, nullptr, nullptr), "NULL argument");
        { dsp_attn_desc d = good.d; d.n_head = 2; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "differ from the handle's"); }
        { dsp_attn_desc d = good.d; d.d_model = 38; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "differ from the handle's"); }
        { dsp_attn_desc d = good.d; d.d_inner = 204; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "differ from the handle's"); }
        { dsp_attn_desc d = good.d; d.d_k = 96; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "differ from the handle's"); }
        { dsp_attn_desc d = good.d; d.d_v = 104; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "differ from the handle's"); }
        { dsp_attn_desc d = good.d; d.eps = 1e-4f; EXPECT(dsp_attn_refresh(keep, &d, nullptr), "eps differs from the handle's"); }
        for (int i = 0; i < DSP_ATTN_PARAMS; ++i) {
            dsp_attn_desc d = good.d;
            d.d_params[i] = nullptr;
            EXPECT(dsp_attn_refresh(keep, &d, nullptr), "NULL parameter tensor");
        }
        EXPECT(dsp_attn_refresh(keep, &good.d, nullptr), "dry_run: launches are refused");
        EXPECT_OK(dsp_attn_destroy(keep));

        // d_model = 1: the forward serves it, training does not
        Block one(1, 4, 4, 4);
        dsp_attn* h1 = nullptr;
        EXPECT_OK(dsp_attn_create(&one.d, &h1));
        if (h1) {
            const char* what = "d_model 1 must be in [2, 64] for training";
            EXPECT_OK(dsp_attn_workspace_bytes(h1, 5, 3, &bytes));
            EXPECT(dsp_attn_tape_bytes(h1, 5, 3, &tape), what);
            EXPECT(dsp_attn_backward_bytes(h1, 5, 3, &wk, &da), what);
            EXPECT(dsp_attn_forward_train(h1, x, 5, 3, y, buf, 1 << 20, nullptr), what);
            EXPECT(dsp_attn_backward(h1, 5, 3, buf, 1 << 20, x, y, buf, 1 << 20, buf, 1 << 20, nullptr), what);
            EXPECT_OK(dsp_attn_destroy(h1));
        }
    } else {
        std::printf("no handle was created\n");
        ++g_bad;
    }

    alignas(16) static float yy[16], W[16], bW[4], v[4], c[1], out[4];
    EXPECT(dsp_selfattn_pool_batch(nullptr, 1, 1, 4, W, bW, v, c, out, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, nullptr, bW, v, c, out, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W, nullptr, v, c, out, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W, bW, nullptr, c, out, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W, bW, v, nullptr, out, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W, bW, v, c, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_batch(yy, 0, 1, 4, W, bW, v, c, out, nullptr), "T 0 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_batch(yy, 1025, 1, 4, W, bW, v, c, out, nullptr), "T 1025 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 0, 4, W, bW, v, c, out, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 0, W, bW, v, c, out, nullptr), "H 0 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 6, W, bW, v, c, out, nullptr), "H 6 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 260, W, bW, v, c, out, nullptr), "H 260 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_batch(yy + 1, 1, 1, 4, W, bW, v, c, out, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W + 1, bW, v, c, out, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_batch(yy, 1, 1, 4, W, bW, v, c, out, nullptr), "dry_run: launches are refused");

    alignas(16) static float w1[4], go[4], gy[4], gp[4], ge[4], gv[4];
    EXPECT(dsp_selfattn_pool_train_batch(nullptr, 1, 1, 4, W, bW, v, c, out, w1, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 1, 1, 4, W, bW, v, c, nullptr, w1, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 1, 1, 4, W, bW, v, c, out, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 0, 1, 4, W, bW, v, c, out, w1, nullptr), "T 0 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 1, 0, 4, W, bW, v, c, out, w1, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 1, 1, 6, W, bW, v, c, out, w1, nullptr), "H 6 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_train_batch(yy + 1, 1, 1, 4, W, bW, v, c, out, w1, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_train_batch(yy, 1, 1, 4, W, bW, v, c, out, w1, nullptr), "dry_run: launches are refused");
    EXPECT(dsp_selfattn_pool_backward_batch(nullptr, 1, 1, 4, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, nullptr, bW, v, w1, go, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, nullptr, v, w1, go, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, nullptr, w1, go, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, nullptr, go, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, nullptr, gy, gp, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go, gy, nullptr, ge, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go, gy, gp, nullptr, gv, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go, gy, gp, ge, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1025, 1, 4, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "T 1025 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 0, 4, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 260, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "H 260 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_backward_batch(yy + 1, 1, 1, 4, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W + 1, bW, v, w1, go, gy, gp, ge, gv, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go + 1, gy, gp, ge, gv, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go, gy, gp, ge, gv, nullptr), "dry_run: launches are refused");
    EXPECT(dsp_selfattn_pool_backward_batch(yy, 1, 1, 4, W, bW, v, w1, go, nullptr, gp, ge, gv, nullptr), "dry_run: launches are refused");   // d_gy is optional

    dsp_debug_host_dry_run(0);
    return finish("asan_attn_args");
}
