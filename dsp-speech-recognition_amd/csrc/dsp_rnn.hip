// The recurrent entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_hmlstm_*, dsp_bigru_*): argument checks,
// packed-parameter handles and launches of the kernels of kernels_hmlstm*.h / kernels_bigru*.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "dsp_common.h"
#include "workspace.h"
#include "dsp_host.h"
#include "kernels_hmlstm.h"
#include "kernels_hmlstm_bwd.h"
#include "kernels_bigru.h"
#include "kernels_bigru_bwd.h"

// Packed parameters of one HM-LSTM (include/dsp_frontend.h: dsp_hmlstm); immutable after dsp_hmlstm_create.
struct dsp_hmlstm {
    int32_t I, H1, H2;
    float* d_packed;       // one allocation: cell 1 W_01 | U_21 | U_11 | bias, cell 2 W_01 | U_11 | bias (kernels_hmlstm.h layout)
    HmCell c1, c2;
    const float4* wt[4];   // in the same allocation: U_11(2)^T, W_01(2)^T, U_21^T, U_11(1)^T (kernels_hmlstm_bwd.h layout)
    int device;
};

// Packed parameters of one bidirectional GRU encoder (include/dsp_frontend.h: dsp_bigru); immutable after dsp_bigru_create.
struct dsp_bigru {
    int32_t I, H, L;
    float* d_packed;       // one allocation: per layer and direction the concatenated [W_ih | W_hh] tiles, then the bias (kernels_bigru.h layout)
    GruDir dir[GRU_MAX_LAYERS][2];
    const float4* wt[GRU_MAX_LAYERS][2];   // in the same allocation: weight_hh^T per layer and direction (kernels_bigru_bwd.h layout)
    int32_t ngx[GRU_MAX_LAYERS], ng[GRU_MAX_LAYERS];
    int device;
};

namespace {

// f(std::integral_constant<int, MAXS>) for the smallest MAXS of 2 / 4 / 7 / MAX tiles per wave that holds nt tiles over 8 waves.
template <int MAX, class F>
void rnn_dispatch_tiles(int nt, F&& f) {
    if (nt <= 2 * HM_WAVES) f(std::integral_constant<int, 2>{});
    else if (nt <= 4 * HM_WAVES) f(std::integral_constant<int, 4>{});
    else if (nt <= 7 * HM_WAVES) f(std::integral_constant<int, 7>{});
    else f(std::integral_constant<int, MAX>{});
}

// Raises the dynamic-LDS limit of kernel K once per device, then launches it with HM_THREADS threads.
template <auto K, class P>
int rnn_launch_dynamic_lds(const char* who, dim3 grid, size_t lds, hipStream_t st, const P& p) {
    static size_t granted[DSP_MAX_DEVICES] = {};        // one per instantiation, i.e. per kernel
    if (dsp_ensure_dynamic_lds((const void*)K, lds, granted) != 0)
        return dsp_fail(DSP_EHIP, "%s: %zu bytes of LDS were not granted", who, lds);
    K<<<grid, HM_THREADS, lds, st>>>(p);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int rnn_check_tb(const char* who, int32_t T, int32_t B) {
    if (T < 1 || B < 1) return dsp_fail(DSP_EINVAL, "%s: T %d and B %d must be >= 1", who, T, B);
    return DSP_OK;
}

// The tape argument of the training entry points: `held` bytes at d_tape against the `need` bytes that `bytes_fn` reports.
// Without a handle (the caller reports that next) `need` is the smallest tape any handle asks for at (T, B).
int rnn_check_tape(const char* who, const void* d_tape, int64_t held, int64_t need, const char* bytes_fn) {
    if (!d_tape) return dsp_fail(DSP_EINVAL, "%s: NULL tape", who);
    if ((reinterpret_cast<uintptr_t>(d_tape) & 15) != 0) return dsp_fail(DSP_EINVAL, "%s: d_tape must be 16-byte aligned", who);
    if (held < need)
        return dsp_fail(DSP_EINVAL, "%s: the tape is short (%lld bytes, %s asks for %lld)", who, (long long)held, bytes_fn, (long long)need);
    return DSP_OK;
}

// The packed-parameter buffer of a handle: reserve() hands out offsets, alloc() makes the one allocation, run() launches the
// pack kernels on stream 0 up to the first error, finish() waits for them and frees the buffer on failure.
struct RnnPacked {
    size_t total = 0;
    float* buf = nullptr;
    hipError_t err = hipSuccess;

    size_t reserve(size_t floats) { return (total += floats) - floats; }
    int alloc() {
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), total * sizeof(float)));
        // the parameters may have been written on any stream of the caller: create is rare, so it simply waits for the device
        err = hipDeviceSynchronize();
        return DSP_OK;
    }
    template <class F>
    void run(F&& launch) {
        if (err == hipSuccess) { launch(); err = hipGetLastError(); }
    }
    int finish(const char* who) {
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess) return DSP_OK;
        (void)hipFree(buf);
        return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(err));
    }
    const float4* f4(size_t off) const { return reinterpret_cast<const float4*>(buf + off); }
};

inline int pack_blocks(int64_t n) { return (int)((n + 255) / 256); }

// Where the pieces of a handle's packed buffer lie, and the pack launches that fill them: what create runs on stream 0 and
// refresh on the caller's stream, into the same places.
struct HmSeg { const float* src; int32_t H, K; };
struct HmLayout {
    HmSeg segs[5], tsegs[4];       // (source, H of the cell, K) in packing order; the transposed copies of the backward recurrence
    size_t off[5], boff[2], toff[4];
};
inline int64_t hm_seg_floats(const HmSeg& s) { return (int64_t)hm_kgroups(s.K) * hm_tiles(s.H) * 256; }

void hmlstm_layout(const dsp_hmlstm_desc* d, RnnPacked& pk, HmLayout& lay) {
    const int32_t I = d->input_size, H1 = d->hidden1, H2 = d->hidden2;
    const HmSeg segs[5] = {{d->d_c1_W01, H1, I}, {d->d_c1_U21, H1, H2}, {d->d_c1_U11, H1, H1}, {d->d_c2_W01, H2, H1}, {d->d_c2_U11, H2, H2}};
    // the transposed copies of the backward recurrence: (source, H of the cell, columns = hidden index of the product)
    const HmSeg tsegs[4] = {{d->d_c2_U11, H2, H2}, {d->d_c2_W01, H2, H1}, {d->d_c1_U21, H1, H2}, {d->d_c1_U11, H1, H1}};
    for (int i = 0; i < 5; ++i) { lay.segs[i] = segs[i]; lay.off[i] = pk.reserve((size_t)hm_seg_floats(segs[i])); }
    lay.boff[0] = pk.reserve((size_t)hm_tiles(H1) * 16);
    lay.boff[1] = pk.reserve((size_t)hm_tiles(H2) * 16);
    for (int i = 0; i < 4; ++i) { lay.tsegs[i] = tsegs[i]; lay.toff[i] = pk.reserve((size_t)hm_bwd_packed_floats(tsegs[i].H, tsegs[i].K)); }
}

void hmlstm_pack(const dsp_hmlstm_desc* d, const HmLayout& lay, RnnPacked& pk, float* buf, hipStream_t st) {
    const int32_t H1 = d->hidden1, H2 = d->hidden2;
    for (int i = 0; i < 5; ++i)
        pk.run([&] {
            const HmSeg& g = lay.segs[i];
            hm_pack_kernel<<<pack_blocks(hm_seg_floats(g)), 256, 0, st>>>(g.src, g.H, g.K, hm_kgroups(g.K), buf + lay.off[i]);
        });
    pk.run([&] { hm_pack_bias_kernel<<<pack_blocks(hm_tiles(H1) * 16), 256, 0, st>>>(d->d_c1_bias, H1, buf + lay.boff[0]); });
    pk.run([&] { hm_pack_bias_kernel<<<pack_blocks(hm_tiles(H2) * 16), 256, 0, st>>>(d->d_c2_bias, H2, buf + lay.boff[1]); });
    for (int i = 0; i < 4; ++i)
        pk.run([&] {
            const HmSeg& g = lay.tsegs[i];
            hm_pack_t_kernel<<<pack_blocks(hm_bwd_packed_floats(g.H, g.K)), 256, 0, st>>>(g.src, g.H, g.K, HM_WAVES * hm_bwd_chunks(g.K),
                                                                                         buf + lay.toff[i]);
        });
}

struct GruLayout {
    size_t woff[GRU_MAX_LAYERS][2], boff[GRU_MAX_LAYERS][2], toff[GRU_MAX_LAYERS][2];
    int32_t ngx[GRU_MAX_LAYERS], ng[GRU_MAX_LAYERS];
};

void bigru_layout(int32_t I, int32_t H, int32_t L, RnnPacked& pk, GruLayout& lay) {
    const int32_t nt = H / 4;
    for (int l = 0; l < L; ++l) {
        lay.ngx[l] = hm_kgroups(l == 0 ? I : 2 * H);
        lay.ng[l] = lay.ngx[l] + hm_kgroups(H);
        for (int dr = 0; dr < 2; ++dr) lay.woff[l][dr] = pk.reserve((size_t)lay.ng[l] * nt * 256);
    }
    for (int l = 0; l < L; ++l)
        for (int dr = 0; dr < 2; ++dr) lay.boff[l][dr] = pk.reserve((size_t)4 * H);
    for (int l = 0; l < L; ++l)       // the transposed copies of the backward recurrence
        for (int dr = 0; dr < 2; ++dr) lay.toff[l][dr] = pk.reserve((size_t)gru_bwd_packed_floats(H));
}

void bigru_pack(const dsp_bigru_desc* d, int32_t I, int32_t H, int32_t L, const GruLayout& lay, RnnPacked& pk, float* buf, hipStream_t st) {
    const int32_t nt = H / 4;
    for (int l = 0; l < L; ++l)
        for (int dr = 0; dr < 2; ++dr)
            pk.run([&] {
                const float* const* p = d->d_params + 8 * l + 4 * dr;      // weight_ih, weight_hh, bias_ih, bias_hh
                gru_pack_kernel<<<pack_blocks((int64_t)lay.ng[l] * nt * 256), 256, 0, st>>>(p[0], p[1], H, l == 0 ? I : 2 * H, lay.ngx[l], lay.ng[l],
                                                                                          buf + lay.woff[l][dr]);
                gru_pack_bias_kernel<<<pack_blocks(4 * H), 256, 0, st>>>(p[2], p[3], H, buf + lay.boff[l][dr]);
                gru_pack_t_kernel<<<pack_blocks(gru_bwd_packed_floats(H)), 256, 0, st>>>(p[1], H, HM_WAVES * hm_bwd_chunks(H), buf + lay.toff[l][dr]);
            });
}

// dsp_*_refresh launches on the handle's device only.
int rnn_check_refresh(const char* who, int device) {
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != device) return dsp_fail(DSP_EINVAL, "%s: the handle belongs to device %d, current device is %d", who, device, dev);
    return DSP_OK;
}

template <class H>
int rnn_destroy(const char* who, H* h) {
    if (!h) return DSP_OK;
    hipError_t e = hipFree(h->d_packed);
    delete h;
    if (e != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(e));
    return DSP_OK;
}

int64_t hmlstm_tape_need(const dsp_hmlstm* h, int32_t T, int32_t B) {
    return hm_tape_floats(h ? h->H1 : 4, h ? h->H2 : 4, T, B) * (int64_t)sizeof(float);
}
int64_t bigru_tape_need(const dsp_bigru* h, int32_t T, int32_t B) {
    return gru_tape_floats(h ? h->H : 4, h ? h->L : 1, T, B) * (int64_t)sizeof(float);
}

// The checks and the launch behind dsp_hmlstm_forward (d_tape == NULL) and dsp_hmlstm_forward_train[_rows] (d_rows: the row
// bound's word or NULL; the training mode alone reads it).
int hmlstm_forward_launch(const char* who, const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a,
                          const int32_t* d_len, const int32_t* d_rows, const float* d_state_in, float* d_state_out, float* d_h1,
                          float* d_h2, uint8_t* d_z1, uint8_t* d_z2, float* d_zhat, float* d_last_h2, float* d_tape, void* stream) {
    if (!h || !d_x) return dsp_fail(DSP_EINVAL, "%s: NULL handle / input", who);
    if (int rc = rnn_check_tb(who, T, B)) return rc;
    if (!std::isfinite(a)) return dsp_fail(DSP_EINVAL, "%s: the slope a is not finite", who);
    if ((reinterpret_cast<uintptr_t>(d_x) & 15) != 0) return dsp_fail(DSP_EINVAL, "%s: d_x must be 16-byte aligned", who);
    if (!d_state_out && !d_h1 && !d_h2 && !d_z1 && !d_z2 && !d_zhat && !d_last_h2)
        return dsp_fail(DSP_EINVAL, "%s: nothing to write (every output is NULL)", who);
    HmParams P;
    P.c1 = h->c1; P.c2 = h->c2;
    P.I = h->I; P.T = T; P.B = B; P.a = a;
    P.x = d_x; P.len = d_len; P.state_in = d_state_in; P.state_out = d_state_out;
    P.h1 = d_h1; P.h2 = d_h2; P.z1 = d_z1; P.z2 = d_z2; P.zhat = d_zhat; P.last_h2 = d_last_h2; P.tape = d_tape; P.rows = d_rows;
    const int grid = hm_slices(B);
    const int nt = h->c1.n_tiles > h->c2.n_tiles ? h->c1.n_tiles : h->c2.n_tiles;
    hipStream_t st = (hipStream_t)stream;
    if (d_tape) rnn_dispatch_tiles<9>(nt, [&](auto m) { hmlstm_forward_kernel<decltype(m)::value, true><<<grid, HM_THREADS, 0, st>>>(P); });
    else rnn_dispatch_tiles<9>(nt, [&](auto m) { hmlstm_forward_kernel<decltype(m)::value><<<grid, HM_THREADS, 0, st>>>(P); });
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

// dsp_hmlstm_forward_train and dsp_hmlstm_forward_train_rows (d_rows may be NULL: the plain call)
int hmlstm_forward_train(const char* who, const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                         const int32_t* d_rows, const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2, uint8_t* d_z1,
                         uint8_t* d_z2, float* d_zhat, float* d_last_h2, void* d_tape, int64_t tape_bytes, void* stream) {
    if (int rc = rnn_check_tb(who, T, B)) return rc;
    if (int rc = rnn_check_tape(who, d_tape, tape_bytes, hmlstm_tape_need(h, T, B), "dsp_hmlstm_tape_bytes")) return rc;
    if (!d_h1 || !d_h2 || !d_z1 || !d_z2) return dsp_fail(DSP_EINVAL, "%s: h1, h2, z1 and z2 are mandatory (the backward pass reads them)", who);
    if (!d_x) return dsp_fail(DSP_EINVAL, "%s: NULL input", who);
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL handle", who);
    return hmlstm_forward_launch(who, h, d_x, T, B, a, d_len, d_rows, d_state_in, d_state_out, d_h1, d_h2, d_z1, d_z2, d_zhat,
                                 d_last_h2, static_cast<float*>(d_tape), stream);
}

// dsp_hmlstm_backward and dsp_hmlstm_backward_rows, the same way
int hmlstm_backward(const char* who, const dsp_hmlstm* h, int32_t T, int32_t B, float a, const int32_t* d_len, const int32_t* d_rows,
                    const float* d_state_in, const void* d_tape, int64_t tape_bytes, const float* d_h1, const float* d_h2,
                    const uint8_t* d_z1, const uint8_t* d_z2, const float* d_g_h1, const float* d_g_h2, const float* d_g_last,
                    float* d_dfs1, float* d_dfs2, void* stream) {
    if (int rc = rnn_check_tb(who, T, B)) return rc;
    if (!std::isfinite(a)) return dsp_fail(DSP_EINVAL, "%s: the slope a is not finite", who);
    if (int rc = rnn_check_tape(who, d_tape, tape_bytes, hmlstm_tape_need(h, T, B), "dsp_hmlstm_tape_bytes")) return rc;
    if (!d_h1 || !d_h2 || !d_z1 || !d_z2) return dsp_fail(DSP_EINVAL, "%s: NULL forward output (h1, h2, z1, z2)", who);
    if (!d_g_h1 && !d_g_h2 && !d_g_last) return dsp_fail(DSP_EINVAL, "%s: no gradient to propagate (g_h1, g_h2 and g_last are all NULL)", who);
    if (!d_dfs1 || !d_dfs2) return dsp_fail(DSP_EINVAL, "%s: NULL output (dfs1, dfs2)", who);
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL handle", who);
    HmBwdParams P;
    for (int i = 0; i < 4; ++i) P.wt[i] = h->wt[i];
    P.H1 = h->H1; P.H2 = h->H2; P.T = T; P.B = B; P.a = a;
    P.len = d_len; P.state_in = d_state_in; P.tape = static_cast<const float*>(d_tape);
    P.h1 = d_h1; P.h2 = d_h2; P.z1 = d_z1; P.z2 = d_z2;
    P.g_h1 = d_g_h1; P.g_h2 = d_g_h2; P.g_last = d_g_last; P.dfs1 = d_dfs1; P.dfs2 = d_dfs2; P.rows = d_rows;
    const dim3 grid(hm_slices(B));
    const size_t lds = hm_bwd_lds_bytes(h->H1, h->H2);       // up to 67.5 KB: above the static limit
    hipStream_t st = (hipStream_t)stream;
    if (hm_bwd_chunks(h->H1 > h->H2 ? h->H1 : h->H2) <= 1) return rnn_launch_dynamic_lds<hmlstm_backward_kernel<1>>(who, grid, lds, st, P);
    return rnn_launch_dynamic_lds<hmlstm_backward_kernel<2>>(who, grid, lds, st, P);
}

int64_t bigru_buffer_floats(const dsp_bigru* h, int32_t T, int32_t B) { return (int64_t)T * B * 2 * h->H; }

// where layer l's output rows and gates start in the tape
float* bigru_tape_rows(const dsp_bigru* h, void* tape, int l, int32_t T, int32_t B) {
    return static_cast<float*>(tape) + l * gru_tape_rows_floats(h->H, T, B);
}
float* bigru_tape_gates(const dsp_bigru* h, void* tape, int l, int32_t T, int32_t B) {
    return static_cast<float*>(tape) + h->L * gru_tape_rows_floats(h->H, T, B) + l * gru_tape_layer_gates_floats(h->H, T, B);
}

// One layer of the forward pass: the plain instantiations, or (tape != NULL) those that also save the gates.
void bigru_launch_layer(const dsp_bigru* h, int l, GruParams& P, float* tape, const float* drop, dim3 grid, hipStream_t st) {
    P.d[0] = h->dir[l][0]; P.d[1] = h->dir[l][1];
    P.I = l == 0 ? h->I : 2 * h->H; P.H = h->H; P.ngx = h->ngx[l]; P.ng = h->ng[l];
    P.tape = tape; P.drop = drop;
    const int nt = h->H / 4;
    if (tape) rnn_dispatch_tiles<8>(nt, [&](auto m) { bigru_layer_kernel<decltype(m)::value, true><<<grid, HM_THREADS, 0, st>>>(P); });
    else rnn_dispatch_tiles<8>(nt, [&](auto m) { bigru_layer_kernel<decltype(m)::value><<<grid, HM_THREADS, 0, st>>>(P); });
}

}  // namespace

extern "C" {

int dsp_hmlstm_create(const dsp_hmlstm_desc* d, dsp_hmlstm** out) {
    if (!d || !out) return dsp_fail(DSP_EINVAL, "dsp_hmlstm_create: NULL argument");
    *out = nullptr;
    if (!hm_size_ok(d->input_size) || !hm_size_ok(d->hidden1) || !hm_size_ok(d->hidden2))
        return dsp_fail(DSP_EINVAL, "dsp_hmlstm_create: input_size %d, hidden1 %d, hidden2 %d must be multiples of 4 in [4, %d]",
                        d->input_size, d->hidden1, d->hidden2, HM_MAX_SIZE);
    if (!d->d_c1_U11 || !d->d_c1_U21 || !d->d_c1_W01 || !d->d_c1_bias || !d->d_c2_U11 || !d->d_c2_W01 || !d->d_c2_bias)
        return dsp_fail(DSP_EINVAL, "dsp_hmlstm_create: NULL parameter tensor");
    const int32_t I = d->input_size, H1 = d->hidden1, H2 = d->hidden2;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    RnnPacked pk;
    HmLayout lay;
    hmlstm_layout(d, pk, lay);
    if (int rc = pk.alloc()) return rc;
    float* buf = pk.buf;
    hmlstm_pack(d, lay, pk, buf, 0);
    if (int rc = pk.finish("dsp_hmlstm_create")) return rc;
    dsp_hmlstm* h = new dsp_hmlstm();
    h->I = I; h->H1 = H1; h->H2 = H2; h->d_packed = buf; h->device = dev;
    h->c1 = HmCell{{pk.f4(lay.off[0]), pk.f4(lay.off[1]), pk.f4(lay.off[2])}, buf + lay.boff[0], {hm_kgroups(I), hm_kgroups(H2), hm_kgroups(H1)}, H1, hm_tiles(H1)};
    h->c2 = HmCell{{pk.f4(lay.off[3]), nullptr, pk.f4(lay.off[4])}, buf + lay.boff[1], {hm_kgroups(H1), 0, hm_kgroups(H2)}, H2, hm_tiles(H2)};
    for (int i = 0; i < 4; ++i) h->wt[i] = pk.f4(lay.toff[i]);
    *out = h;
    return DSP_OK;
}

int dsp_hmlstm_destroy(dsp_hmlstm* h) { return rnn_destroy("dsp_hmlstm_destroy", h); }

int dsp_hmlstm_refresh(dsp_hmlstm* h, const dsp_hmlstm_desc* d, void* stream) {
    const char* who = "dsp_hmlstm_refresh";
    if (!h || !d) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (d->input_size != h->I || d->hidden1 != h->H1 || d->hidden2 != h->H2)
        return dsp_fail(DSP_EINVAL, "%s: input_size %d, hidden1 %d, hidden2 %d differ from the handle's %d, %d, %d", who, d->input_size,
                        d->hidden1, d->hidden2, h->I, h->H1, h->H2);
    if (!d->d_c1_U11 || !d->d_c1_U21 || !d->d_c1_W01 || !d->d_c1_bias || !d->d_c2_U11 || !d->d_c2_W01 || !d->d_c2_bias)
        return dsp_fail(DSP_EINVAL, "%s: NULL parameter tensor", who);
    if (int rc = rnn_check_refresh(who, h->device)) return rc;
    RnnPacked pk;
    HmLayout lay;
    hmlstm_layout(d, pk, lay);
    hmlstm_pack(d, lay, pk, h->d_packed, (hipStream_t)stream);
    if (pk.err != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(pk.err));
    return DSP_OK;
}

int dsp_hmlstm_forward(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                       const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2, uint8_t* d_z1, uint8_t* d_z2,
                       float* d_zhat, float* d_last_h2, void* stream) {
    return hmlstm_forward_launch("dsp_hmlstm_forward", h, d_x, T, B, a, d_len, nullptr, d_state_in, d_state_out, d_h1, d_h2, d_z1,
                                 d_z2, d_zhat, d_last_h2, nullptr, stream);
}

int dsp_hmlstm_tape_bytes(const dsp_hmlstm* h, int32_t T, int32_t B, int64_t* bytes) {
    if (!h || !bytes) return dsp_fail(DSP_EINVAL, "dsp_hmlstm_tape_bytes: NULL argument");
    if (int rc = rnn_check_tb("dsp_hmlstm_tape_bytes", T, B)) return rc;
    *bytes = hmlstm_tape_need(h, T, B);
    return DSP_OK;
}

int dsp_hmlstm_forward_train(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                             const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2, uint8_t* d_z1, uint8_t* d_z2,
                             float* d_zhat, float* d_last_h2, void* d_tape, int64_t tape_bytes, void* stream) {
    return hmlstm_forward_train("dsp_hmlstm_forward_train", h, d_x, T, B, a, d_len, nullptr, d_state_in, d_state_out, d_h1, d_h2, d_z1,
                                d_z2, d_zhat, d_last_h2, d_tape, tape_bytes, stream);
}

int dsp_hmlstm_forward_train_rows(const dsp_hmlstm* h, const float* d_x, int32_t T, int32_t B, float a, const int32_t* d_len,
                                  const int32_t* d_rows, const float* d_state_in, float* d_state_out, float* d_h1, float* d_h2,
                                  uint8_t* d_z1, uint8_t* d_z2, float* d_zhat, float* d_last_h2, void* d_tape, int64_t tape_bytes,
                                  void* stream) {
    return hmlstm_forward_train("dsp_hmlstm_forward_train_rows", h, d_x, T, B, a, d_len, d_rows, d_state_in, d_state_out, d_h1, d_h2,
                                d_z1, d_z2, d_zhat, d_last_h2, d_tape, tape_bytes, stream);
}

int dsp_hmlstm_backward(const dsp_hmlstm* h, int32_t T, int32_t B, float a, const int32_t* d_len, const float* d_state_in,
                        const void* d_tape, int64_t tape_bytes, const float* d_h1, const float* d_h2, const uint8_t* d_z1,
                        const uint8_t* d_z2, const float* d_g_h1, const float* d_g_h2, const float* d_g_last, float* d_dfs1,
                        float* d_dfs2, void* stream) {
    return hmlstm_backward("dsp_hmlstm_backward", h, T, B, a, d_len, nullptr, d_state_in, d_tape, tape_bytes, d_h1, d_h2, d_z1, d_z2,
                           d_g_h1, d_g_h2, d_g_last, d_dfs1, d_dfs2, stream);
}

int dsp_hmlstm_backward_rows(const dsp_hmlstm* h, int32_t T, int32_t B, float a, const int32_t* d_len, const int32_t* d_rows,
                             const float* d_state_in, const void* d_tape, int64_t tape_bytes, const float* d_h1, const float* d_h2,
                             const uint8_t* d_z1, const uint8_t* d_z2, const float* d_g_h1, const float* d_g_h2,
                             const float* d_g_last, float* d_dfs1, float* d_dfs2, void* stream) {
    return hmlstm_backward("dsp_hmlstm_backward_rows", h, T, B, a, d_len, d_rows, d_state_in, d_tape, tape_bytes, d_h1, d_h2, d_z1, d_z2,
                           d_g_h1, d_g_h2, d_g_last, d_dfs1, d_dfs2, stream);
}

int dsp_bigru_create(const dsp_bigru_desc* d, dsp_bigru** out) {
    if (!d || !out) return dsp_fail(DSP_EINVAL, "dsp_bigru_create: NULL argument");
    *out = nullptr;
    const int32_t I = d->input_size, H = d->hidden, L = d->n_layers;
    if (I < 1 || I > GRU_MAX_IN) return dsp_fail(DSP_EINVAL, "dsp_bigru_create: input_size %d must be in [1, %d]", I, GRU_MAX_IN);
    if (H < 4 || H > GRU_MAX_H || (H & 3) != 0)
        return dsp_fail(DSP_EINVAL, "dsp_bigru_create: hidden %d must be a multiple of 4 in [4, %d]", H, GRU_MAX_H);
    if (L < 1 || L > GRU_MAX_LAYERS) return dsp_fail(DSP_EINVAL, "dsp_bigru_create: n_layers %d must be in [1, %d]", L, GRU_MAX_LAYERS);
    for (int i = 0; i < 8 * L; ++i)
        if (!d->d_params[i]) return dsp_fail(DSP_EINVAL, "dsp_bigru_create: NULL parameter tensor (index %d)", i);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    RnnPacked pk;
    GruLayout lay;
    bigru_layout(I, H, L, pk, lay);
    if (int rc = pk.alloc()) return rc;
    float* buf = pk.buf;
    bigru_pack(d, I, H, L, lay, pk, buf, 0);
    if (int rc = pk.finish("dsp_bigru_create")) return rc;
    dsp_bigru* h = new dsp_bigru();
    h->I = I; h->H = H; h->L = L; h->d_packed = buf; h->device = dev;
    for (int l = 0; l < L; ++l) {
        h->ngx[l] = lay.ngx[l]; h->ng[l] = lay.ng[l];
        for (int dr = 0; dr < 2; ++dr) {
            h->dir[l][dr] = GruDir{pk.f4(lay.woff[l][dr]), buf + lay.boff[l][dr]};
            h->wt[l][dr] = pk.f4(lay.toff[l][dr]);
        }
    }
    *out = h;
    return DSP_OK;
}

int dsp_bigru_destroy(dsp_bigru* h) { return rnn_destroy("dsp_bigru_destroy", h); }

int dsp_bigru_refresh(dsp_bigru* h, const dsp_bigru_desc* d, void* stream) {
    const char* who = "dsp_bigru_refresh";
    if (!h || !d) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (d->input_size != h->I || d->hidden != h->H || d->n_layers != h->L)
        return dsp_fail(DSP_EINVAL, "%s: input_size %d, hidden %d, n_layers %d differ from the handle's %d, %d, %d", who, d->input_size,
                        d->hidden, d->n_layers, h->I, h->H, h->L);
    for (int i = 0; i < 8 * h->L; ++i)
        if (!d->d_params[i]) return dsp_fail(DSP_EINVAL, "%s: NULL parameter tensor (index %d)", who, i);
    if (int rc = rnn_check_refresh(who, h->device)) return rc;
    RnnPacked pk;
    GruLayout lay;
    bigru_layout(h->I, h->H, h->L, pk, lay);
    bigru_pack(d, h->I, h->H, h->L, lay, pk, h->d_packed, (hipStream_t)stream);
    if (pk.err != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(pk.err));
    return DSP_OK;
}

int dsp_bigru_workspace_bytes(const dsp_bigru* h, int32_t T, int32_t B, int64_t* bytes) {
    if (!h || !bytes) return dsp_fail(DSP_EINVAL, "dsp_bigru_workspace_bytes: NULL argument");
    if (int rc = rnn_check_tb("dsp_bigru_workspace_bytes", T, B)) return rc;
    *bytes = (h->L > 1 ? 2 : 1) * bigru_buffer_floats(h, T, B) * (int64_t)sizeof(float);
    return DSP_OK;
}

int dsp_bigru_forward(const dsp_bigru* h, const float* d_x, int32_t T, int32_t B, const int32_t* d_len, float* d_y,
                      float* d_hn, void* d_work, int64_t work_bytes, void* stream) {
    if (!h || !d_x) return dsp_fail(DSP_EINVAL, "dsp_bigru_forward: NULL handle / input");
    if (int rc = rnn_check_tb("dsp_bigru_forward", T, B)) return rc;
    if (!d_y && !d_hn) return dsp_fail(DSP_EINVAL, "dsp_bigru_forward: nothing to write (d_y and d_hn are NULL)");
    const int64_t per = bigru_buffer_floats(h, T, B), need = (h->L > 1 ? 2 : 1) * per * (int64_t)sizeof(float);
    if (!d_work || work_bytes < need)
        return dsp_fail(DSP_EINVAL, "dsp_bigru_forward: the workspace holds %lld bytes, %lld are needed", (long long)(d_work ? work_bytes : 0),
                        (long long)need);
    if ((reinterpret_cast<uintptr_t>(d_work) & 3) != 0) return dsp_fail(DSP_EINVAL, "dsp_bigru_forward: d_work must be 4-byte aligned");
    float* bufs[2] = {static_cast<float*>(d_work), static_cast<float*>(d_work) + (h->L > 1 ? per : 0)};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(hm_slices(B), 2);
    for (int l = 0; l < h->L; ++l) {
        const bool last = l == h->L - 1;
        GruParams P;
        P.T = T; P.B = B;
        P.x = l == 0 ? d_x : bufs[(l - 1) & 1];
        P.len = d_len;
        P.out = (last && !d_y) ? nullptr : bufs[l & 1];
        P.hn = d_hn ? d_hn + (int64_t)2 * l * B * h->H : nullptr;
        bigru_launch_layer(h, l, P, nullptr, nullptr, grid, st);
        HIP_TRY(hipGetLastError());
    }
    if (d_y) {
        bigru_sum_kernel<<<grid_for((int64_t)T * B * h->H, 256), 256, 0, st>>>(bufs[(h->L - 1) & 1], d_len, T, B, h->H, d_y);
        HIP_TRY(hipGetLastError());
    }
    return DSP_OK;
}

int dsp_bigru_tape_bytes(const dsp_bigru* h, int32_t T, int32_t B, int64_t* bytes) {
    if (!h || !bytes) return dsp_fail(DSP_EINVAL, "dsp_bigru_tape_bytes: NULL argument");
    if (int rc = rnn_check_tb("dsp_bigru_tape_bytes", T, B)) return rc;
    *bytes = bigru_tape_need(h, T, B);
    return DSP_OK;
}

int dsp_bigru_tape_rows(const dsp_bigru* h, int32_t layer, int32_t T, int32_t B, int64_t* offset_bytes) {
    if (!h || !offset_bytes) return dsp_fail(DSP_EINVAL, "dsp_bigru_tape_rows: NULL argument");
    if (int rc = rnn_check_tb("dsp_bigru_tape_rows", T, B)) return rc;
    if (layer < 0 || layer >= h->L) return dsp_fail(DSP_EINVAL, "dsp_bigru_tape_rows: layer %d out of range [0, %d)", layer, h->L);
    *offset_bytes = layer * gru_tape_rows_floats(h->H, T, B) * (int64_t)sizeof(float);
    return DSP_OK;
}

int dsp_bigru_forward_train(const dsp_bigru* h, const float* d_x, int32_t T, int32_t B, const int32_t* d_len, const float* d_drop,
                            float* d_y, float* d_hn, void* d_tape, int64_t tape_bytes, void* stream) {
    const char* who = "dsp_bigru_forward_train";
    if (int rc = rnn_check_tb(who, T, B)) return rc;
    if (int rc = rnn_check_tape(who, d_tape, tape_bytes, bigru_tape_need(h, T, B), "dsp_bigru_tape_bytes")) return rc;
    if (!d_x) return dsp_fail(DSP_EINVAL, "%s: NULL input", who);
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL handle", who);
    if ((reinterpret_cast<uintptr_t>(d_drop) & 3) != 0) return dsp_fail(DSP_EINVAL, "%s: d_drop must be 4-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(hm_slices(B), 2);
    for (int l = 0; l < h->L; ++l) {
        GruParams P;
        P.T = T; P.B = B;
        P.x = l == 0 ? d_x : bigru_tape_rows(h, d_tape, l - 1, T, B);
        P.len = d_len;
        P.out = bigru_tape_rows(h, d_tape, l, T, B);
        P.hn = d_hn ? d_hn + (int64_t)2 * l * B * h->H : nullptr;
        bigru_launch_layer(h, l, P, bigru_tape_gates(h, d_tape, l, T, B),
                           (l > 0 && d_drop) ? d_drop + (int64_t)(l - 1) * gru_tape_rows_floats(h->H, T, B) : nullptr, grid, st);
        HIP_TRY(hipGetLastError());
    }
    if (d_y) {
        bigru_sum_kernel<<<grid_for((int64_t)T * B * h->H, 256), 256, 0, st>>>(bigru_tape_rows(h, d_tape, h->L - 1, T, B), d_len, T, B, h->H, d_y);
        HIP_TRY(hipGetLastError());
    }
    return DSP_OK;
}

int dsp_bigru_backward(const dsp_bigru* h, int32_t layer, int32_t T, int32_t B, const int32_t* d_len, const void* d_tape,
                       int64_t tape_bytes, const float* d_g, const float* d_g_hn, float* d_da, void* stream) {
    const char* who = "dsp_bigru_backward";
    if (int rc = rnn_check_tb(who, T, B)) return rc;
    if (int rc = rnn_check_tape(who, d_tape, tape_bytes, bigru_tape_need(h, T, B), "dsp_bigru_tape_bytes")) return rc;
    if (!d_g && !d_g_hn) return dsp_fail(DSP_EINVAL, "%s: no gradient to propagate (g and g_hn are both NULL)", who);
    if (!d_da) return dsp_fail(DSP_EINVAL, "%s: NULL output (da)", who);
    if (((reinterpret_cast<uintptr_t>(d_g) | reinterpret_cast<uintptr_t>(d_g_hn) | reinterpret_cast<uintptr_t>(d_da)) & 3) != 0)
        return dsp_fail(DSP_EINVAL, "%s: g, g_hn and da must be 4-byte aligned", who);
    if (!h) return dsp_fail(DSP_EINVAL, "%s: NULL handle", who);
    if (layer < 0 || layer >= h->L) return dsp_fail(DSP_EINVAL, "%s: layer %d out of range [0, %d)", who, layer, h->L);
    GruBwdParams P;
    P.wt[0] = h->wt[layer][0]; P.wt[1] = h->wt[layer][1];
    P.H = h->H; P.T = T; P.B = B;
    P.g_stride = layer == h->L - 1 ? h->H : 2 * h->H;
    P.len = d_len;
    P.gates = bigru_tape_gates(h, const_cast<void*>(d_tape), layer, T, B);
    P.out = bigru_tape_rows(h, const_cast<void*>(d_tape), layer, T, B);
    P.g = d_g; P.g_hn = d_g_hn; P.da = d_da;
    const dim3 grid(hm_slices(B), 2);
    const size_t lds = gru_bwd_lds_bytes(h->H);                // up to 64 KiB: above the static limit
    hipStream_t st = (hipStream_t)stream;
    if (hm_bwd_chunks(h->H) <= 1) return rnn_launch_dynamic_lds<bigru_backward_kernel<1>>(who, grid, lds, st, P);
    return rnn_launch_dynamic_lds<bigru_backward_kernel<2>>(who, grid, lds, st, P);
}

}  // extern "C"
