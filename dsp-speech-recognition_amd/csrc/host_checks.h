// The vocabulary of the host-side argument checks, one definition each (included through dsp_host.h): alignment, address
// ranges and their overlap, the named collector behind "the outputs lie apart from each other and from everything read",
// and the refusal of a launch under dsp_debug_host_dry_run.  Sizes are in BYTES; NULL is the empty range.  Host only.
#pragma once

#include <stdint.h>

namespace {

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

struct Range {
    uintptr_t lo, hi;       // [lo, hi)
};

// NULL -> the empty range {0, 0}, which overlaps nothing.
Range range_of(const void* p, int64_t bytes) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return p ? Range{lo, lo + (uintptr_t)bytes} : Range{0, 0};
}

bool overlap(Range a, Range b) { return a.lo < b.hi && b.lo < a.hi; }

// The outputs must lie apart from each other and from everything that is read (inputs may share memory).  Reports the first
// offending pair in the order of the add() calls, the later-added name first.
struct Ranges {
    struct Named {
        const char* name;
        Range span;
        bool output;
    } r[24];
    int k = 0;
    void add(const char* name, const void* p, int64_t bytes, bool output) {
        if (p) r[k++] = Named{name, range_of(p, bytes), output};
    }
    int check(const char* who) const {
        for (int i = 0; i < k; ++i)
            for (int j = i + 1; j < k; ++j)
                if ((r[i].output || r[j].output) && overlap(r[i].span, r[j].span))
                    return dsp_fail(DSP_EINVAL, "%s: %s overlaps %s", who, r[j].name, r[i].name);
        return DSP_OK;
    }
};

// The same rule for callers that name the output first: every output against every input, then against the outputs behind it.
int check_overlaps(const char* who, const Range* outs, const char* const* out_names, int n_out, const Range* ins,
                   const char* const* in_names, int n_in) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (overlap(outs[o], ins[i])) return dsp_fail(DSP_EINVAL, "%s: %s overlaps %s", who, out_names[o], in_names[i]);
        for (int q = o + 1; q < n_out; ++q)
            if (overlap(outs[o], outs[q])) return dsp_fail(DSP_EINVAL, "%s: %s overlaps %s", who, out_names[o], out_names[q]);
    }
    return DSP_OK;
}

// What passed every check is refused instead of launched on a thread under dsp_debug_host_dry_run (it has no device), or with a
// handle made under it (`handle_dry_run`).  `who` NULL: the two callers whose message carries no entry-point name.
int dsp_refuse_dry_run(const char* who, int handle_dry_run = 0) {
    if (!g_host_dry_run && !handle_dry_run) return DSP_OK;
    return dsp_fail(DSP_EINVAL, "%s%sdry_run: launches are refused under dsp_debug_host_dry_run", who ? who : "", who ? ": " : "");
}

}  // namespace
