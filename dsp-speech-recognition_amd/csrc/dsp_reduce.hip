// The row-bounded column sums of libdsp_frontend.so and the census of a recorded graph (include/dsp_frontend.h:
// dsp_rows_colsum_scratch_bytes, dsp_rows_colsum, dsp_graph_census): argument checks, the launches of kernels_reduce.h, and a
// host-only walk over a hipGraph_t.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <string.h>

#include <vector>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_reduce.h"
#include "rows_host.h"

extern "C" {

int dsp_rows_colsum_scratch_bytes(int32_t T, int32_t B, int32_t cols, int64_t* out_bytes) {
    const char* who = "dsp_rows_colsum_scratch_bytes";
    if (!out_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = check_sizes(who, T, B)) return rc;
    if (cols < 1 || cols > WGRAD_MAX_DIM) return dsp_fail(DSP_EINVAL, "%s: cols %d must be in [1, %d]", who, cols, WGRAD_MAX_DIM);
    *out_bytes = colsum_scratch_floats(T, B, cols) * 4;
    return DSP_OK;
}

int dsp_rows_colsum(const dsp_rows_operand* a, const dsp_rows_operand* x, int32_t T, int32_t B, const int32_t* d_rows, float* d_out,
                    void* d_scratch, int64_t scratch_bytes, void* stream) {
    const char* who = "dsp_rows_colsum";
    if (int rc = check_sizes(who, T, B)) return rc;
    RowsOp A, X = {};
    Range ra, rx{0, 0};
    if (int rc = check_operand(who, "a", a, T, B, &A, &ra)) return rc;
    if (x) {
        if (int rc = check_operand(who, "x", x, T, B, &X, &rx)) return rc;
        if (X.cols != A.cols) return dsp_fail(DSP_EINVAL, "%s: operand x has %d columns, operand a %d", who, X.cols, A.cols);
    }
    if (!d_out) return dsp_fail(DSP_EINVAL, "%s: NULL output d_out", who);
    if (!d_scratch) return dsp_fail(DSP_EINVAL, "%s: NULL scratch", who);
    if (!aligned(d_out, 4) || (d_rows && !aligned(d_rows, 4))) return dsp_fail(DSP_EINVAL, "%s: every pointer must be 4-byte aligned", who);
    if (!aligned(d_scratch, 16)) return dsp_fail(DSP_EINVAL, "%s: scratch must be 16-byte aligned", who);
    const int32_t cols = A.cols;
    const int64_t need = colsum_scratch_floats(T, B, cols) * 4;
    if (scratch_bytes < need)
        return dsp_fail(DSP_EINVAL, "%s: scratch of %lld bytes is short of the %lld dsp_rows_colsum_scratch_bytes asks for", who,
                        (long long)scratch_bytes, (long long)need);
    // output and scratch against everything that is read, and against each other
    const Range outs[2] = {range_of(d_out, cols * 4), range_of(d_scratch, need)};
    const char* out_names[2] = {"d_out", "scratch"};
    const Range ins[3] = {ra, rx, range_of(d_rows, 4)};
    const char* in_names[3] = {"operand a", "operand x", "d_rows"};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 3; ++i)
            if (overlap(outs[o], ins[i])) return dsp_fail(DSP_EINVAL, "%s: %s overlaps %s", who, out_names[o], in_names[i]);
    if (overlap(outs[0], outs[1])) return dsp_fail(DSP_EINVAL, "%s: d_out overlaps scratch", who);
    if (int rc = dsp_refuse_dry_run(who)) return rc;

    hipStream_t st = (hipStream_t)stream;
    const int steps = wgrad_chunk_steps(B);
    const int chunks = (T + steps - 1) / steps;
    float* part = static_cast<float*>(d_scratch);
    const dim3 grid(colsum_col_blocks(cols), chunks);
    if (cols >= COLSUM_WIDE_MIN)
        rows_colsum_wide_kernel<<<grid, COLSUM_THREADS, 0, st>>>(A, X, x != nullptr, T, B, d_rows, part);
    else
        rows_colsum_narrow_kernel<<<grid, COLSUM_THREADS, 0, st>>>(A, X, x != nullptr, T, B, d_rows, part);
    HIP_TRY(hipGetLastError());
    rows_colsum_reduce_kernel<<<dim3((cols + 255) / 256), 256, 0, st>>>(part, cols, T, B, d_rows, d_out);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_graph_census(void* hip_graph, dsp_graph_census_t* out, char* names, size_t names_bytes) {
    const char* who = "dsp_graph_census";
    if (!out) return dsp_fail(DSP_EINVAL, "%s: NULL output", who);
    if (!names && names_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL names with names_bytes %zu", who, names_bytes);
    if (!hip_graph) return dsp_fail(DSP_EINVAL, "%s: NULL graph", who);
    hipGraph_t graph = static_cast<hipGraph_t>(hip_graph);
    memset(out, 0, sizeof(*out));
    if (names) names[0] = '\0';

    size_t n = 0;
    HIP_TRY(hipGraphGetNodes(graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) HIP_TRY(hipGraphGetNodes(graph, nodes.data(), &n));
    size_t roots = 0;
    HIP_TRY(hipGraphGetRootNodes(graph, nullptr, &roots));
    out->n_nodes = (int32_t)n;
    out->n_roots = (int32_t)roots;
    size_t used = 0;                                                       // bytes of `names` written, terminator excluded
    int64_t wanted = 1;                                                    // bytes every name needs, terminator included
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType type;
        HIP_TRY(hipGraphNodeGetType(nodes[i], &type));
        size_t fan = 0;
        HIP_TRY(hipGraphNodeGetDependentNodes(nodes[i], nullptr, &fan));
        if ((int64_t)fan > out->max_fanout) out->max_fanout = (int32_t)fan;
        if (type == hipGraphNodeTypeKernel) {
            ++out->n_kernel;
            hipKernelNodeParams kp;
            memset(&kp, 0, sizeof(kp));
            const char* name = nullptr;
            if (hipGraphKernelNodeGetParams(nodes[i], &kp) == hipSuccess && kp.func) name = hipKernelNameRefByPtr(kp.func, nullptr);
            (void)hipGetLastError();                                       // a node without parameters is reported as "?"
            if (!name) name = "?";
            const size_t len = strlen(name);
            wanted += (int64_t)len + 1;
            if (names && used + len + 2 <= names_bytes) {                  // the name, a newline, the terminator
                memcpy(names + used, name, len);
                names[used + len] = '\n';
                used += len + 1;
                names[used] = '\0';
            }
        } else if (type == hipGraphNodeTypeMemset) {
            ++out->n_memset;
            hipMemsetParams mp;
            memset(&mp, 0, sizeof(mp));
            HIP_TRY(hipGraphMemsetNodeGetParams(nodes[i], &mp));
            const int64_t bytes = (int64_t)mp.elementSize * (int64_t)mp.width * (int64_t)(mp.height ? mp.height : 1);
            if (bytes > 4) ++out->n_wide_memset;
            if (bytes > out->widest_memset_bytes) out->widest_memset_bytes = bytes;
        } else if (type == hipGraphNodeTypeMemcpy) {
            ++out->n_memcpy;
        } else {
            ++out->n_other;
        }
    }
    out->names_bytes = wanted;
    return DSP_OK;
}

}  // extern "C"
