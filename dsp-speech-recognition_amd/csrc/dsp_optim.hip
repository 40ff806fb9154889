// The optimiser entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_adam_*): argument checks, the chunk table, the
// handle of a device-resident Adam and the launches of kernels_optim.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_optim.h"

// include/dsp_frontend.h: dsp_adam.  The tables are immutable after create but for the gradient pointers and the state.
struct dsp_adam {
    int32_t n;
    AdamTables tb;          // device addresses (host addresses for a dry-run handle)
    void* blob;             // the one allocation they point into
    std::vector<int64_t> numel;
    std::vector<uintptr_t> pmv;   // 3n: the addresses create checked, for bind's overlap check
    int bound;              // dsp_adam_bind_grads has been called
    int device;             // -1 for a dry-run handle
    int dry_run;            // tables in HOST memory (dsp_debug_host_dry_run): the handle can be destroyed, nothing else
};

namespace {

struct AdamRange {
    uintptr_t lo, hi;       // [lo, hi)
    int32_t tensor;
    char what;              // 'p', 'm', 'v', 'g'
};

// Sorts the ranges and names the first two that share a byte.
int adam_check_disjoint(const char* who, std::vector<AdamRange>& r) {
    std::sort(r.begin(), r.end(), [](const AdamRange& a, const AdamRange& b) { return a.lo < b.lo; });
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i].lo < r[i - 1].hi)
            return dsp_fail(DSP_EINVAL, "%s: %c[%d] and %c[%d] overlap", who, r[i - 1].what, r[i - 1].tensor, r[i].what, r[i].tensor);
    return DSP_OK;
}

int adam_check_hyper(const char* who, double lr, double beta1, double beta2, double eps) {
    if (!std::isfinite(lr)) return dsp_fail(DSP_EINVAL, "%s: lr is not finite", who);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return dsp_fail(DSP_EINVAL, "%s: beta1 %g must be in [0, 1)", who, beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return dsp_fail(DSP_EINVAL, "%s: beta2 %g must be in [0, 1)", who, beta2);
    if (!(eps >= 0.0) || !std::isfinite(eps)) return dsp_fail(DSP_EINVAL, "%s: eps %g must be finite and >= 0", who, eps);
    return DSP_OK;
}

int adam_check_numel(const char* who, int32_t n, const int64_t* numel) {
    if (n <= 0) return dsp_fail(DSP_EINVAL, "%s: n %d must be >= 1", who, n);
    for (int32_t t = 0; t < n; ++t)
        if (numel[t] <= 0 || numel[t] > (int64_t)1 << 40)
            return dsp_fail(DSP_EINVAL, "%s: numel[%d] %lld must be in [1, 2^40]", who, t, (long long)numel[t]);
    return DSP_OK;
}

int64_t adam_count_chunks(int32_t n, const int64_t* numel) {
    int64_t total = 0;
    for (int32_t t = 0; t < n; ++t) total += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
    return total;
}

void adam_fill_chunks(int32_t n, const int64_t* numel, int32_t* tensor, int64_t* offset) {
    int64_t k = 0;
    for (int32_t t = 0; t < n; ++t)
        for (int64_t off = 0; off < numel[t]; off += ADAM_CHUNK, ++k) {
            tensor[k] = t;
            offset[k] = off;
        }
}

// A handle a launch may use: not a dry-run one, and of the current device.
int adam_check_usable(const char* who, const dsp_adam* h) {
    if (h->dry_run) return dsp_fail(DSP_EINVAL, "%s: the handle was created under dsp_debug_host_dry_run: launches are refused", who);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return dsp_fail(DSP_EINVAL, "%s: the handle belongs to device %d, current device is %d", who, h->device, dev);
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_adam_chunk_elems(void) { return ADAM_CHUNK; }

int dsp_adam_chunk_table(int32_t n, const int64_t* numel, int64_t capacity, int32_t* tensor, int64_t* offset, int64_t* n_chunks) {
    const char* who = "dsp_adam_chunk_table";
    if (!numel || !n_chunks) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    *n_chunks = 0;
    if (int rc = adam_check_numel(who, n, numel)) return rc;
    const int64_t total = adam_count_chunks(n, numel);
    *n_chunks = total;
    if (!tensor && !offset) return DSP_OK;             // the count alone
    if (!tensor || !offset) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (capacity < total) return dsp_fail(DSP_EINVAL, "%s: capacity %lld is below the %lld chunks", who, (long long)capacity, (long long)total);
    adam_fill_chunks(n, numel, tensor, offset);
    return DSP_OK;
}

int dsp_adam_create(int32_t n, const int64_t* numel, float* const* d_p, float* const* d_m, float* const* d_v, double lr, double beta1,
                    double beta2, double eps, dsp_adam** out) {
    const char* who = "dsp_adam_create";
    if (!out) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    if (!numel || !d_p || !d_m || !d_v) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = adam_check_numel(who, n, numel)) return rc;
    if (int rc = adam_check_hyper(who, lr, beta1, beta2, eps)) return rc;
    std::vector<AdamRange> ranges;
    ranges.reserve((size_t)3 * n);
    for (int32_t t = 0; t < n; ++t) {
        float* const three[3] = {d_p[t], d_m[t], d_v[t]};
        for (int k = 0; k < 3; ++k) {
            if (!three[k]) return dsp_fail(DSP_EINVAL, "%s: NULL pointer %c[%d]", who, "pmv"[k], t);
            const uintptr_t lo = reinterpret_cast<uintptr_t>(three[k]);
            if (lo & 3) return dsp_fail(DSP_EINVAL, "%s: %c[%d] is not 4-byte aligned", who, "pmv"[k], t);
            ranges.push_back({lo, lo + (uintptr_t)numel[t] * 4, t, "pmv"[k]});
        }
    }
    std::vector<uintptr_t> pmv;
    pmv.reserve(ranges.size());
    for (const AdamRange& r : ranges) pmv.push_back(r.lo);     // (t, k) order, before the sort
    if (int rc = adam_check_disjoint(who, ranges)) return rc;

    // one blob: state | p [n] | m [n] | v [n] | g [n] | numel [n] | chunk_off [nc] | chunk_tensor [nc]
    const int64_t nc = adam_count_chunks(n, numel);
    const size_t o_p = sizeof(AdamState), o_m = o_p + (size_t)n * 8, o_v = o_m + (size_t)n * 8, o_g = o_v + (size_t)n * 8,
                 o_numel = o_g + (size_t)n * 8, o_off = o_numel + (size_t)n * 8, o_ten = o_off + (size_t)nc * 8,
                 bytes = o_ten + (size_t)nc * 4;
    static_assert(sizeof(AdamState) % 8 == 0, "the pointer tables behind the state must stay 8-byte aligned");
    std::vector<unsigned char> host(bytes, 0);
    AdamState st;
    std::memset(&st, 0, sizeof st);
    st.lr = lr; st.beta1 = beta1; st.beta2 = beta2; st.eps = eps;
    std::memcpy(host.data(), &st, sizeof st);
    std::memcpy(host.data() + o_p, d_p, (size_t)n * 8);
    std::memcpy(host.data() + o_m, d_m, (size_t)n * 8);
    std::memcpy(host.data() + o_v, d_v, (size_t)n * 8);
    std::memcpy(host.data() + o_numel, numel, (size_t)n * 8);
    adam_fill_chunks(n, numel, reinterpret_cast<int32_t*>(host.data() + o_ten), reinterpret_cast<int64_t*>(host.data() + o_off));

    int dev = -1;
    if (!g_host_dry_run) HIP_TRY(hipGetDevice(&dev));
    void* blob = nullptr;
    const hipError_t e = dsp_table_alloc_copy(&blob, host.data(), bytes);
    if (e != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(e));
    unsigned char* b = static_cast<unsigned char*>(blob);
    dsp_adam* h = new dsp_adam();
    h->n = n;
    h->blob = blob;
    h->tb.state = reinterpret_cast<AdamState*>(b);
    h->tb.p = reinterpret_cast<float* const*>(b + o_p);
    h->tb.m = reinterpret_cast<float* const*>(b + o_m);
    h->tb.v = reinterpret_cast<float* const*>(b + o_v);
    h->tb.g = reinterpret_cast<float* const*>(b + o_g);
    h->tb.numel = reinterpret_cast<const int64_t*>(b + o_numel);
    h->tb.chunk_off = reinterpret_cast<const int64_t*>(b + o_off);
    h->tb.chunk_tensor = reinterpret_cast<const int32_t*>(b + o_ten);
    h->tb.n_chunks = nc;
    h->numel.assign(numel, numel + n);
    h->pmv = std::move(pmv);
    h->bound = 0;
    h->device = dev;
    h->dry_run = g_host_dry_run ? 1 : 0;
    *out = h;
    return DSP_OK;
}

int dsp_adam_destroy(dsp_adam* h) {
    if (!h) return DSP_OK;
    dsp_table_free(h->blob, h->dry_run);
    delete h;
    return DSP_OK;
}

int dsp_adam_bind_grads(dsp_adam* h, float* const* d_g, void* stream) {
    const char* who = "dsp_adam_bind_grads";
    if (!h || !d_g) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    std::vector<AdamRange> ranges;
    ranges.reserve((size_t)4 * h->n);
    for (int32_t t = 0; t < h->n; ++t) {
        if (!d_g[t]) return dsp_fail(DSP_EINVAL, "%s: NULL pointer g[%d]", who, t);
        const uintptr_t lo = reinterpret_cast<uintptr_t>(d_g[t]);
        if (lo & 3) return dsp_fail(DSP_EINVAL, "%s: g[%d] is not 4-byte aligned", who, t);
        const uintptr_t len = (uintptr_t)h->numel[t] * 4;
        ranges.push_back({lo, lo + len, t, 'g'});
        for (int k = 0; k < 3; ++k) ranges.push_back({h->pmv[(size_t)3 * t + k], h->pmv[(size_t)3 * t + k] + len, t, "pmv"[k]});
    }
    if (int rc = adam_check_disjoint(who, ranges)) return rc;
    if (int rc = adam_check_usable(who, h)) return rc;
    float** table = const_cast<float**>(h->tb.g);
    for (int32_t first = 0; first < h->n; first += ADAM_BIND_BATCH) {
        AdamPtrBatch batch;
        const int32_t count = std::min<int32_t>(ADAM_BIND_BATCH, h->n - first);
        for (int32_t i = 0; i < ADAM_BIND_BATCH; ++i) batch.ptr[i] = i < count ? d_g[first + i] : nullptr;
        adam_bind_kernel<<<1, 64, 0, (hipStream_t)stream>>>(table, batch, first, count);
        HIP_TRY(hipGetLastError());
    }
    h->bound = 1;
    return DSP_OK;
}

int dsp_adam_set_hyper(dsp_adam* h, double lr, double beta1, double beta2, double eps, void* stream) {
    const char* who = "dsp_adam_set_hyper";
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = adam_check_hyper(who, lr, beta1, beta2, eps)) return rc;
    if (int rc = adam_check_usable(who, h)) return rc;
    adam_set_hyper_kernel<<<1, 1, 0, (hipStream_t)stream>>>(h->tb.state, lr, beta1, beta2, eps);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_adam_set_step(dsp_adam* h, int64_t step, void* stream) {
    const char* who = "dsp_adam_set_step";
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (step < 0) return dsp_fail(DSP_EINVAL, "%s: step %lld must be >= 0", who, (long long)step);
    if (int rc = adam_check_usable(who, h)) return rc;
    adam_set_step_kernel<<<1, 1, 0, (hipStream_t)stream>>>(h->tb.state, (long long)step);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_adam_get_state(const dsp_adam* h, int64_t* step, double* hyper, void* stream) {
    const char* who = "dsp_adam_get_state";
    if (!h || !step || !hyper) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = adam_check_usable(who, h)) return rc;
    AdamState st;
    HIP_TRY(hipMemcpyAsync(&st, h->tb.state, sizeof st, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *step = st.step;
    hyper[0] = st.lr; hyper[1] = st.beta1; hyper[2] = st.beta2; hyper[3] = st.eps;
    return DSP_OK;
}

int dsp_adam_step(dsp_adam* h, int32_t zero_grads, void* stream) {
    const char* who = "dsp_adam_step";
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (!h->bound) return dsp_fail(DSP_EINVAL, "%s: no gradients are bound (dsp_adam_bind_grads)", who);
    if (int rc = adam_check_usable(who, h)) return rc;
    hipStream_t st = (hipStream_t)stream;
    adam_advance_kernel<<<1, 1, 0, st>>>(h->tb.state);
    HIP_TRY(hipGetLastError());
    const int grid = grid_for(h->tb.n_chunks, 1);
    if (zero_grads) adam_step_kernel<true><<<grid, ADAM_THREADS, 0, st>>>(h->tb);
    else adam_step_kernel<false><<<grid, ADAM_THREADS, 0, st>>>(h->tb);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // extern "C"
