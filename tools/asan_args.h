// The harness of the stand-alone sanitized check programs (tools/asan_*_args.cpp): one count of failures, EXPECT (a call must
// return DSP_EINVAL with a message that holds the given text), EXPECT_OK (a call must return DSP_OK), and finish(), through
// which every program ends: it prints "<name>: ok" or "<name>: <n> FAILED" and returns the exit status.
// With DSP_ASAN_ARGS_TRANSCRIPT set in the environment, every EXPECT / EXPECT_OK also prints its source line, the return code
// and the complete dsp_last_error() text: two builds of the library give the same transcript exactly when they answer every
// call of the program with the same code and the same message, byte for byte.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dsp_frontend.h"

static int g_bad = 0;

static inline void transcript(int rc, int line) {
    static const bool on = std::getenv("DSP_ASAN_ARGS_TRANSCRIPT") != nullptr;
    if (!on) return;
    const char* e = dsp_last_error();
    std::printf("transcript line %d: rc %d: %s\n", line, rc, e ? e : "(none)");
}

static inline void expect(int rc, const char* what, int line) {
    transcript(rc, line);
    const char* e = dsp_last_error();
    if (rc != DSP_EINVAL || !e || !std::strstr(e, what)) {
        std::printf("line %d: rc %d, message '%s', expected DSP_EINVAL with '%s'\n", line, rc, e ? e : "(none)", what);
        ++g_bad;
    }
}

static inline void expect_ok(int rc, int line) {
    transcript(rc, line);
    if (rc != DSP_OK) {
        const char* e = dsp_last_error();
        std::printf("line %d: rc %d, message '%s', expected DSP_OK\n", line, rc, e ? e : "(none)");
        ++g_bad;
    }
}

#define EXPECT(call, what) expect((call), (what), __LINE__)
#define EXPECT_OK(call) expect_ok((call), __LINE__)

static inline int finish(const char* name) {
    if (g_bad) {
        std::printf("%s: %d FAILED\n", name, g_bad);
        return 1;
    }
    std::printf("%s: ok\n", name);
    return 0;
}
