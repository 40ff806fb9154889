// Stand-alone host check of the head entry points (include/dsp_frontend.h: dsp_head_lengths_batch, dsp_head_pool_batch,
// dsp_head_pool_train_batch, dsp_head_pool_backward_batch; csrc/dsp_head.hip; and dsp_selfattn_pool_rows_batch with its training
// twins dsp_selfattn_pool_rows_train_batch / dsp_selfattn_pool_rows_backward_batch, csrc/dsp_attn.hip).  Every argument error
// is DSP_EINVAL with a message before any device call, and under dsp_debug_host_dry_run(1) what passed every check is refused instead of launched: the
// program needs no GPU.  `make -C dsp-speech-recognition_amd/csrc asan-head` builds it with AddressSanitizer + UBSan against the
// sanitized build of the library and runs it; it needs no preloaded runtime.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "asan_args.h"
#include "dsp_frontend.h"

int main() {
    dsp_debug_host_dry_run(1);
    const char* refused = "dry_run: launches are refused";
    // never reached by a kernel: every call below returns before a launch
    alignas(16) static float y[16], feat[16], W[16], bW[4], v[4], c[1], out[4];
    static int32_t len[4] = {1, 2, 3, 4}, len0c[4], len1[4], info[4], rows[1] = {1};

    EXPECT(dsp_head_lengths_batch(nullptr, 4, 200, 5, len0c, len1, info, nullptr), "NULL argument");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 5, nullptr, len1, info, nullptr), "NULL argument");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 5, len0c, nullptr, info, nullptr), "NULL argument");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 5, len0c, len1, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_head_lengths_batch(len, 0, 200, 5, len0c, len1, info, nullptr), "B 0 must be in [1, 65535]");
    EXPECT(dsp_head_lengths_batch(len, -3, 200, 5, len0c, len1, info, nullptr), "B -3 must be in [1, 65535]");
    EXPECT(dsp_head_lengths_batch(len, 65536, 200, 5, len0c, len1, info, nullptr), "B 65536 must be in [1, 65535]");
    EXPECT(dsp_head_lengths_batch(len, 4, 0, 5, len0c, len1, info, nullptr), "T 0 must be >= 1");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 0, len0c, len1, info, nullptr), "hir 0 must be >= 1");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, -1, len0c, len1, info, nullptr), "hir -1 must be >= 1");
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 5, len0c, len1, info, nullptr), refused);
    EXPECT(dsp_head_lengths_batch(len, 4, 200, 1, len, len1, info, nullptr), refused);             // in place
    EXPECT(dsp_head_lengths_batch(len, 65535, 0x7fffffff, 0x7fffffff, len0c, len1, info, nullptr), refused);

    EXPECT(dsp_head_pool_batch(nullptr, 2, 1, 4, len, rows, feat, 8, 0, 4, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, nullptr, rows, feat, 8, 0, 4, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, nullptr, 8, 0, 4, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_batch(y, 0, 1, 4, len, rows, feat, 8, 0, 4, nullptr), "T 0 must be >= 1");
    EXPECT(dsp_head_pool_batch(y, 2, 0, 4, len, rows, feat, 8, 0, 4, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 0, len, rows, feat, 8, 0, 4, nullptr), "H 0 must be in [1, 4194240]");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4194241, len, rows, feat, 1 << 24, 0, 4194241, nullptr), "H 4194241 must be in [1, 4194240]");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 8, 0, -1, nullptr), "col_max -1 is negative");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 8, 0, 3, nullptr), "overlap");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 8, 2, 0, nullptr), "overlap");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 8, 4, 4, nullptr), "overlap");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 7, 0, 4, nullptr), "ld_feat 7 is below the 8 columns written");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 7, 4, 0, nullptr), "ld_feat 7 is below the 8 columns written");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 3, -1, 0, nullptr), "ld_feat 3 is below the 4 columns written");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 0x7ffffff0, 0x7ffffff0, 0, nullptr), "ld_feat 2147483632 is below the 2147483636 columns written");
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 8, 0, 4, nullptr), refused);
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, nullptr, feat, 8, 4, 0, nullptr), refused);        // d_rows is optional
    EXPECT(dsp_head_pool_batch(y, 2, 1, 4, len, rows, feat, 4, -1, 0, nullptr), refused);          // no average
    EXPECT(dsp_head_pool_batch(y + 1, 2, 1, 3, len, rows, feat, 16, 9, 1, nullptr), refused);      // the scalar route

    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, bW, v, c, out, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(nullptr, 1, 1, 4, W, bW, v, c, out, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, nullptr, bW, v, c, out, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, nullptr, v, c, out, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, bW, nullptr, c, out, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, bW, v, nullptr, out, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, bW, v, c, nullptr, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 0, 1, 4, W, bW, v, c, out, rows, nullptr), "T 0 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1025, 1, 4, W, bW, v, c, out, rows, nullptr), "T 1025 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 0, 4, W, bW, v, c, out, rows, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 6, W, bW, v, c, out, rows, nullptr), "H 6 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_rows_batch(y + 1, 1, 1, 4, W, bW, v, c, out, rows, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W + 1, bW, v, c, out, rows, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_rows_batch(y, 1, 1, 4, W, bW, v, c, out, rows, nullptr), refused);

    // the training twins: dsp_head_pool_train_batch, dsp_head_pool_backward_batch, dsp_selfattn_pool_rows_{train,backward}_batch
    static int32_t arg[4];
    alignas(16) static float gy[16], w1[4], gp[16], ge[4], gv[4];
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, feat, 8, 0, 4, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_train_batch(nullptr, 2, 1, 4, len, rows, feat, 8, 0, 4, arg, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, nullptr, rows, feat, 8, 0, 4, arg, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, nullptr, 8, 0, 4, arg, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_train_batch(y, 0, 1, 4, len, rows, feat, 8, 0, 4, arg, nullptr), "T 0 must be >= 1");
    EXPECT(dsp_head_pool_train_batch(y, 2, 0, 4, len, rows, feat, 8, 0, 4, arg, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 0, len, rows, feat, 8, 0, 4, arg, nullptr), "H 0 must be in [1, 4194240]");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, feat, 8, 0, -1, arg, nullptr), "col_max -1 is negative");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, feat, 8, 2, 0, arg, nullptr), "overlap");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, feat, 7, 0, 4, arg, nullptr), "ld_feat 7 is below the 8 columns written");
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, rows, feat, 8, 0, 4, arg, nullptr), refused);
    EXPECT(dsp_head_pool_train_batch(y, 2, 1, 4, len, nullptr, feat, 4, -1, 0, arg, nullptr), refused);   // d_rows is optional, no average
    EXPECT(dsp_head_pool_train_batch(y + 1, 2, 1, 3, len, rows, feat, 16, 9, 1, arg, nullptr), refused);  // the scalar route

    EXPECT(dsp_head_pool_backward_batch(nullptr, 8, 0, 4, len, arg, 2, 1, 4, gy, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, nullptr, arg, 2, 1, 4, gy, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, nullptr, 2, 1, 4, gy, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, arg, 2, 1, 4, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, arg, 0, 1, 4, gy, nullptr), "T 0 must be >= 1");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, arg, 2, 0, 4, gy, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, arg, 2, 1, 0, gy, nullptr), "H 0 must be in [1, 4194240]");
    EXPECT(dsp_head_pool_backward_batch(feat, 1 << 24, 0, 4194241, len, arg, 2, 1, 4194241, gy, nullptr), "H 4194241 must be in [1, 4194240]");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, -1, len, arg, 2, 1, 4, gy, nullptr), "col_max -1 is negative");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 3, len, arg, 2, 1, 4, gy, nullptr), "overlap");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 2, 0, len, arg, 2, 1, 4, gy, nullptr), "overlap");
    EXPECT(dsp_head_pool_backward_batch(feat, 7, 0, 4, len, arg, 2, 1, 4, gy, nullptr), "ld_g 7 is below the 8 columns read");
    EXPECT(dsp_head_pool_backward_batch(feat, 3, -1, 0, len, arg, 2, 1, 4, gy, nullptr), "ld_g 3 is below the 4 columns read");
    EXPECT(dsp_head_pool_backward_batch(feat, 0x7ffffff0, 0x7ffffff0, 0, len, arg, 2, 1, 4, gy, nullptr), "ld_g 2147483632 is below the 2147483636 columns read");
    EXPECT(dsp_head_pool_backward_batch(feat, 8, 0, 4, len, arg, 2, 1, 4, gy, nullptr), refused);
    EXPECT(dsp_head_pool_backward_batch(feat, 4, -1, 0, len, arg, 2, 1, 4, gy, nullptr), refused);        // no average
    EXPECT(dsp_head_pool_backward_batch(feat, 16, 9, 1, len, arg, 2, 1, 3, gy + 1, nullptr), refused);    // the scalar route

    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 1, 4, W, bW, v, c, out, w1, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 1, 4, W, bW, v, c, out, nullptr, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_train_batch(nullptr, 1, 1, 4, W, bW, v, c, out, w1, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 1, 4, W, bW, v, c, nullptr, w1, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1025, 1, 4, W, bW, v, c, out, w1, rows, nullptr), "T 1025 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 0, 4, W, bW, v, c, out, w1, rows, nullptr), "B 0 must be >= 1");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 1, 6, W, bW, v, c, out, w1, rows, nullptr), "H 6 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y + 1, 1, 1, 4, W, bW, v, c, out, w1, rows, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_rows_train_batch(y, 1, 1, 4, W, bW, v, c, out, w1, rows, nullptr), refused);

    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, gy, gp, ge, gv, nullptr, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(nullptr, 1, 1, 4, W, bW, v, w1, out, gy, gp, ge, gv, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, nullptr, out, gy, gp, ge, gv, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, nullptr, gy, gp, ge, gv, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, gy, nullptr, ge, gv, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, gy, gp, nullptr, gv, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, gy, gp, ge, nullptr, rows, nullptr), "NULL argument");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 0, 1, 4, W, bW, v, w1, out, gy, gp, ge, gv, rows, nullptr), "T 0 must be in [1, 1024]");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 260, W, bW, v, w1, out, gy, gp, ge, gv, rows, nullptr), "H 260 must be a multiple of 4 in [4, 256]");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out + 1, gy, gp, ge, gv, rows, nullptr), "must be 16-byte aligned");
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, gy, gp, ge, gv, rows, nullptr), refused);
    EXPECT(dsp_selfattn_pool_rows_backward_batch(y, 1, 1, 4, W, bW, v, w1, out, nullptr, gp, ge, gv, rows, nullptr), refused);   // d_gy is optional

    dsp_debug_host_dry_run(0);
    return finish("asan_head_args");
}
