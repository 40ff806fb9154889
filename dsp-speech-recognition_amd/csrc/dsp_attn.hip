// The attention entry points of libdsp_frontend.so (include/dsp_frontend.h: dsp_attn_*, dsp_selfattn_pool_*): argument
// checks, the packed-parameter handle of a Transformer encoder block and the launches of kernels_attn.h and kernels_attn_bwd.h.  gfx950 / ROCm only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "dsp_common.h"
#include "dsp_host.h"
#include "kernels_attn.h"
#include "kernels_attn_bwd.h"

// Packed parameters of one encoder block (include/dsp_frontend.h: dsp_attn); immutable after dsp_attn_create.
struct dsp_attn {
    int32_t d, d_inner, d_k, d_v;
    float* d_packed;       // one allocation: the six packed matrices of the forward, the six of the backward (kernels_attn_bwd.h:
                           // AttnBwdWeights), then the seven padded vectors (kernels_attn.h: AttnWeights)
    AttnWeights w;
    AttnBwdWeights v;
    int device;            // -1 for a dry-run handle
    int dry_run;           // the packed copy is in HOST memory (dsp_debug_host_dry_run): the handle can be destroyed, nothing else
};

namespace {

int64_t attn_act_floats(const dsp_attn* h, int32_t T, int32_t B) { return (int64_t)B * at_pad16(T) * at_pad16(h->d); }
int64_t attn_stat_floats(int32_t T) { return (int64_t)at_pad16(T) * at_pad16(T); }
int64_t attn_work_bytes(const dsp_attn* h, int32_t T, int32_t B) {
    return 2 * (attn_act_floats(h, T, B) + attn_stat_floats(T)) * (int64_t)sizeof(float);
}

// Training: the tape is the forward's workspace and the rows M behind it; the backward's workspace holds the padded g_M, the
// row part of dx and the statistic D; da holds the seven dense row gradients.
int64_t attn_tape_bytes(const dsp_attn* h, int32_t T, int32_t B) {
    return (3 * attn_act_floats(h, T, B) + 2 * attn_stat_floats(T)) * (int64_t)sizeof(float);
}
int64_t attn_bwd_work_bytes(const dsp_attn* h, int32_t T, int32_t B) {
    return (2 * attn_act_floats(h, T, B) + attn_stat_floats(T)) * (int64_t)sizeof(float);
}
int64_t attn_da_bytes(const dsp_attn* h, int32_t T, int32_t B) {
    return (int64_t)T * B * (4 * h->d + h->d_inner + h->d_v + h->d_k) * (int64_t)sizeof(float);
}

int attn_check_tb(const char* who, int32_t T, int32_t B) {
    if (T < 1 || T > AT_MAX_T) return dsp_fail(DSP_EINVAL, "%s: T %d must be in [1, %d]", who, T, AT_MAX_T);
    if (B < 1) return dsp_fail(DSP_EINVAL, "%s: B %d must be >= 1", who, B);
    if ((int64_t)B * (at_pad16(T) >> 4) > 0x7fffffff) return dsp_fail(DSP_EINVAL, "%s: B %d x T %d is more than one launch holds", who, B, T);
    return DSP_OK;
}

// The training entry points: the sizes of the forward, and a d_model of at least 2 (the unbiased sigma of one element is 0 / 0).
int attn_check_train(const char* who, const dsp_attn* h, int32_t T, int32_t B) {
    if (int rc = attn_check_tb(who, T, B)) return rc;
    if (h->d < 2) return dsp_fail(DSP_EINVAL, "%s: d_model %d must be in [2, %d] for training", who, h->d, AT_MAX_D);
    return DSP_OK;
}

int attn_check_buffer(const char* who, const char* name, const void* p, int64_t have, int64_t need) {
    if (!p || have < need)
        return dsp_fail(DSP_EINVAL, "%s: %s holds %lld bytes, %lld are needed", who, name, (long long)(p ? have : 0), (long long)need);
    if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) return dsp_fail(DSP_EINVAL, "%s: %s must be 16-byte aligned", who, name);
    return DSP_OK;
}

bool mult4_in(int32_t v, int32_t hi) { return v >= 4 && v <= hi && (v & 3) == 0; }

// A handle or call a launch may go ahead with: not under dry run, and on the handle's device.
int attn_check_launch(const char* who, const dsp_attn* h) {
    if (int rc = dsp_refuse_dry_run(who, h && h->dry_run)) return rc;
    if (!h) return DSP_OK;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != h->device) return dsp_fail(DSP_EINVAL, "%s: the handle belongs to device %d, current device is %d", who, h->device, dev);
    return DSP_OK;
}

// The packed buffer of a handle: the 12 matrices as (source, K, N, stride of k, stride of n) -- the last six are the backward's,
// each matrix of the forward the other way round -- and the 7 vectors as (source, n, padded n), with their offsets in floats.
// What dsp_attn_create packs on the host and dsp_attn_refresh gathers on the device, into the same places.
struct AttnMat { const float* src; int32_t K, N; int64_t sk, sn; };
struct AttnVec { const float* src; int32_t n, np; };
struct AttnLayout {
    AttnMat mats[AT_PACK_MATS];
    AttnVec vecs[AT_PACK_VECS];
    size_t moff[AT_PACK_MATS], voff[AT_PACK_VECS], total;
};

void attn_layout(const float* const* p, int32_t d, int32_t di, int32_t dk, int32_t dv, AttnLayout& lay) {
    const int32_t DP = at_pad16(d), IP = at_pad16(di);
    const AttnMat mats[AT_PACK_MATS] = {{p[0], d, dk, dk, 1}, {p[1], dk, d, 1, dk}, {p[2], d, dv, dv, 1},
                                        {p[5], dv, d, 1, dv}, {p[7], d, di, 1, d}, {p[9], di, d, 1, di},
                                        {p[9], d, di, di, 1}, {p[7], di, d, d, 1}, {p[5], d, dv, dv, 1},
                                        {p[2], dv, d, 1, dv}, {p[1], d, dk, dk, 1}, {p[0], dk, d, 1, dk}};
    const AttnVec vecs[AT_PACK_VECS] = {{p[3], d, DP}, {p[4], d, DP}, {p[6], d, DP}, {p[8], di, IP}, {p[10], d, DP}, {p[11], d, DP}, {p[12], d, DP}};
    size_t total = 0;
    for (int i = 0; i < AT_PACK_MATS; ++i) { lay.mats[i] = mats[i]; lay.moff[i] = total; total += (size_t)at_pad16(mats[i].K) * at_pad16(mats[i].N); }
    for (int i = 0; i < AT_PACK_VECS; ++i) { lay.vecs[i] = vecs[i]; lay.voff[i] = total; total += (size_t)vecs[i].np; }
    lay.total = total;
}

}  // namespace

extern "C" {

int dsp_attn_create(const dsp_attn_desc* desc, dsp_attn** out) {
    const char* who = "dsp_attn_create";
    if (!desc || !out) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    const int32_t d = desc->d_model, di = desc->d_inner, dk = desc->d_k, dv = desc->d_v;
    if (desc->n_head != 1) return dsp_fail(DSP_EINVAL, "%s: n_head %d must be 1", who, desc->n_head);
    if (d < 1 || d > AT_MAX_D) return dsp_fail(DSP_EINVAL, "%s: d_model %d must be in [1, %d]", who, d, AT_MAX_D);
    if (!mult4_in(dk, AT_MAX_DKV) || !mult4_in(dv, AT_MAX_DKV))
        return dsp_fail(DSP_EINVAL, "%s: d_k %d and d_v %d must be multiples of 4 in [4, %d]", who, dk, dv, AT_MAX_DKV);
    if (!mult4_in(di, AT_MAX_INNER)) return dsp_fail(DSP_EINVAL, "%s: d_inner %d must be a multiple of 4 in [4, %d]", who, di, AT_MAX_INNER);
    if (!std::isfinite(desc->eps) || desc->eps < 0.f) return dsp_fail(DSP_EINVAL, "%s: eps must be finite and not negative", who);
    for (int i = 0; i < DSP_ATTN_PARAMS; ++i)
        if (!desc->d_params[i]) return dsp_fail(DSP_EINVAL, "%s: NULL parameter tensor (index %d)", who, i);
    // elements of the parameters in the descriptor's order
    const size_t n_el[DSP_ATTN_PARAMS] = {(size_t)d * dk, (size_t)d * dk, (size_t)d * dv, (size_t)d, (size_t)d, (size_t)d * dv, (size_t)d,
                                          (size_t)di * d, (size_t)di, (size_t)d * di, (size_t)d, (size_t)d, (size_t)d};
    int dev = -1;
    std::vector<std::vector<float>> host(DSP_ATTN_PARAMS);
    const float* p[DSP_ATTN_PARAMS];
    if (g_host_dry_run) {
        for (int i = 0; i < DSP_ATTN_PARAMS; ++i) p[i] = desc->d_params[i];      // no device: the tensors are host memory
    } else {
        HIP_TRY(hipGetDevice(&dev));
        // the parameters may have been written on any stream of the caller: create is rare, so it simply waits for the device
        HIP_TRY(hipDeviceSynchronize());
        for (int i = 0; i < DSP_ATTN_PARAMS; ++i) {
            host[i].resize(n_el[i]);
            HIP_TRY(hipMemcpy(host[i].data(), desc->d_params[i], n_el[i] * sizeof(float), hipMemcpyDeviceToHost));
            p[i] = host[i].data();
        }
    }
    const int32_t DP = at_pad16(d), KP = at_pad16(dk), VP = at_pad16(dv), IP = at_pad16(di);
    AttnLayout lay;
    attn_layout(p, d, di, dk, dv, lay);
    const AttnMat* mats = lay.mats;
    const AttnVec* vecs = lay.vecs;
    const size_t *moff = lay.moff, *voff = lay.voff, total = lay.total;
    constexpr int NM = AT_PACK_MATS;
    std::vector<float> blob(total, 0.f);
    for (int i = 0; i < NM; ++i) at_pack_host(blob.data() + moff[i], mats[i].src, mats[i].K, mats[i].N, mats[i].sk, mats[i].sn);
    for (int i = 0; i < AT_PACK_VECS; ++i)
        for (int j = 0; j < vecs[i].n; ++j) blob[voff[i] + j] = vecs[i].src[j];
    void* tables = nullptr;
    const hipError_t e = dsp_table_alloc_copy(&tables, blob.data(), total * sizeof(float));
    if (e != hipSuccess) return dsp_fail(DSP_EHIP, "%s: %s", who, hipGetErrorString(e));
    dsp_attn* h = new dsp_attn();
    h->d = d; h->d_inner = di; h->d_k = dk; h->d_v = dv;
    float* buf = h->d_packed = static_cast<float*>(tables);
    h->dry_run = g_host_dry_run ? 1 : 0;
    h->device = dev;
    auto f4 = [&](int i) { return reinterpret_cast<const float4*>(buf + moff[i]); };
    AttnWeights& w = h->w;
    w.wq = f4(0); w.wkt = f4(1); w.wv = f4(2); w.wpt = f4(3); w.w1t = f4(4); w.w2t = f4(5);
    h->v = AttnBwdWeights{f4(6), f4(7), f4(8), f4(9), f4(10), f4(11)};
    w.ln1a = buf + voff[0]; w.ln1b = buf + voff[1]; w.pb = buf + voff[2]; w.b1 = buf + voff[3]; w.b2 = buf + voff[4];
    w.ln2a = buf + voff[5]; w.ln2b = buf + voff[6];
    w.d = d; w.ngd = DP >> 4; w.ngk = KP >> 4; w.ngv = VP >> 4; w.ngi = IP >> 4;
    w.eps = desc->eps;
    w.inv_temper = (float)(1.0 / std::sqrt((double)d));      // transformer.py:38: temper = d_model ** 0.5
    *out = h;
    return DSP_OK;
}

int dsp_attn_destroy(dsp_attn* h) {
    if (!h) return DSP_OK;
    dsp_table_free(h->d_packed, h->dry_run);
    delete h;
    return DSP_OK;
}

int dsp_attn_refresh(dsp_attn* h, const dsp_attn_desc* desc, void* stream) {
    const char* who = "dsp_attn_refresh";
    if (!h || !desc) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (desc->n_head != 1 || desc->d_model != h->d || desc->d_inner != h->d_inner || desc->d_k != h->d_k || desc->d_v != h->d_v)
        return dsp_fail(DSP_EINVAL, "%s: n_head %d, d_model %d, d_inner %d, d_k %d, d_v %d differ from the handle's 1, %d, %d, %d, %d", who,
                        desc->n_head, desc->d_model, desc->d_inner, desc->d_k, desc->d_v, h->d, h->d_inner, h->d_k, h->d_v);
    if (desc->eps != h->w.eps) return dsp_fail(DSP_EINVAL, "%s: eps differs from the handle's", who);
    for (int i = 0; i < DSP_ATTN_PARAMS; ++i)
        if (!desc->d_params[i]) return dsp_fail(DSP_EINVAL, "%s: NULL parameter tensor (index %d)", who, i);
    if (int rc = attn_check_launch(who, h)) return rc;
    AttnLayout lay;
    attn_layout(desc->d_params, h->d, h->d_inner, h->d_k, h->d_v, lay);
    AtPackJobs J;
    int64_t most = 0;
    for (int i = 0; i < AT_PACK_MATS; ++i) {
        const AttnMat& m = lay.mats[i];
        J.job[i] = AtPackJob{m.src, h->d_packed + lay.moff[i], m.K, m.N, m.sk, m.sn};
        const int64_t n = (int64_t)at_pad16(m.K) * at_pad16(m.N);
        most = n > most ? n : most;
    }
    for (int i = 0; i < AT_PACK_VECS; ++i) {     // K = 0 marks a vector: its n elements are copied, the zero padding behind them stays
        J.job[AT_PACK_MATS + i] = AtPackJob{lay.vecs[i].src, h->d_packed + lay.voff[i], 0, lay.vecs[i].n, 0, 1};
        most = lay.vecs[i].n > most ? lay.vecs[i].n : most;
    }
    attn_pack_kernel<<<dim3((unsigned)((most + 255) / 256), AT_PACK_MATS + AT_PACK_VECS), 256, 0, (hipStream_t)stream>>>(J);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

int dsp_attn_workspace_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* bytes) {
    const char* who = "dsp_attn_workspace_bytes";
    if (!h || !bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = attn_check_tb(who, T, B)) return rc;
    *bytes = attn_work_bytes(h, T, B);
    return DSP_OK;
}

}  // extern "C"

namespace {

// The three launches of the forward; train: d_work is the tape, whose M rows lie behind the forward's workspace.
int attn_launch_forward(const dsp_attn* h, const float* d_x, int32_t T, int32_t B, float* d_y, void* d_work, bool train, void* stream) {
    AttnParams P;
    P.w = h->w;
    P.T = T; P.TP = at_pad16(T); P.B = B;
    P.x = d_x; P.y = d_y;
    P.xp = static_cast<float*>(d_work);
    P.qp = P.xp + attn_act_floats(h, T, B);
    P.smax = P.qp + attn_act_floats(h, T, B);
    P.ssum = P.smax + attn_stat_floats(T);
    P.msave = train ? P.ssum + attn_stat_floats(T) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = P.TP >> 4;
    attn_proj_kernel<<<B * tiles, 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    attn_stats_kernel<<<dim3(tiles, tiles), AT_STAT_WAVES * 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    attn_out_kernel<<<B * tiles, 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_attn_forward(const dsp_attn* h, const float* d_x, int32_t T, int32_t B, float* d_y, void* d_work, int64_t work_bytes,
                     void* stream) {
    const char* who = "dsp_attn_forward";
    if (!h || !d_x || !d_y) return dsp_fail(DSP_EINVAL, "%s: NULL handle / input / output", who);
    if (int rc = attn_check_tb(who, T, B)) return rc;
    const int64_t need = attn_work_bytes(h, T, B);
    if (!d_work || work_bytes < need)
        return dsp_fail(DSP_EINVAL, "%s: the workspace holds %lld bytes, %lld are needed", who, (long long)(d_work ? work_bytes : 0), (long long)need);
    if ((reinterpret_cast<uintptr_t>(d_work) & 15) != 0) return dsp_fail(DSP_EINVAL, "%s: d_work must be 16-byte aligned", who);
    if (int rc = attn_check_launch(who, h)) return rc;
    return attn_launch_forward(h, d_x, T, B, d_y, d_work, false, stream);
}

int dsp_attn_tape_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* bytes) {
    const char* who = "dsp_attn_tape_bytes";
    if (!h || !bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = attn_check_train(who, h, T, B)) return rc;
    *bytes = attn_tape_bytes(h, T, B);
    return DSP_OK;
}

int dsp_attn_forward_train(const dsp_attn* h, const float* d_x, int32_t T, int32_t B, float* d_y, void* d_tape, int64_t tape_bytes,
                           void* stream) {
    const char* who = "dsp_attn_forward_train";
    if (!h || !d_x || !d_y) return dsp_fail(DSP_EINVAL, "%s: NULL handle / input / output", who);
    if (int rc = attn_check_train(who, h, T, B)) return rc;
    if (int rc = attn_check_buffer(who, "d_tape", d_tape, tape_bytes, attn_tape_bytes(h, T, B))) return rc;
    if (int rc = attn_check_launch(who, h)) return rc;
    return attn_launch_forward(h, d_x, T, B, d_y, d_tape, true, stream);
}

int dsp_attn_backward_bytes(const dsp_attn* h, int32_t T, int32_t B, int64_t* work_bytes, int64_t* da_bytes) {
    const char* who = "dsp_attn_backward_bytes";
    if (!h || !work_bytes || !da_bytes) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (int rc = attn_check_train(who, h, T, B)) return rc;
    *work_bytes = attn_bwd_work_bytes(h, T, B);
    *da_bytes = attn_da_bytes(h, T, B);
    return DSP_OK;
}

int dsp_attn_backward(const dsp_attn* h, int32_t T, int32_t B, const void* d_tape, int64_t tape_bytes, const float* d_gy, float* d_gx,
                      float* d_da, int64_t da_bytes, void* d_work, int64_t work_bytes, void* stream) {
    const char* who = "dsp_attn_backward";
    if (!h || !d_gy) return dsp_fail(DSP_EINVAL, "%s: NULL handle / gradient", who);
    if (int rc = attn_check_train(who, h, T, B)) return rc;
    if (int rc = attn_check_buffer(who, "d_tape", d_tape, tape_bytes, attn_tape_bytes(h, T, B))) return rc;
    if (int rc = attn_check_buffer(who, "d_work", d_work, work_bytes, attn_bwd_work_bytes(h, T, B))) return rc;
    const int64_t da_need = attn_da_bytes(h, T, B);
    if (!d_da || da_bytes < da_need)
        return dsp_fail(DSP_EINVAL, "%s: d_da holds %lld bytes, %lld are needed", who, (long long)(d_da ? da_bytes : 0), (long long)da_need);
    if (int rc = attn_check_launch(who, h)) return rc;
    AttnBwdParams P;
    P.w = h->w; P.v = h->v;
    P.T = T; P.TP = at_pad16(T); P.B = B;
    P.di = h->d_inner; P.dk = h->d_k; P.dv = h->d_v;
    const int64_t act = attn_act_floats(h, T, B), stat = attn_stat_floats(T), rows = (int64_t)T * B;
    const float* tape = static_cast<const float*>(d_tape);
    P.xp = tape; P.qp = P.xp + act; P.smax = P.qp + act; P.ssum = P.smax + stat; P.mp = P.ssum + stat;
    P.gy = d_gy; P.gx = d_gx;
    P.g_r2 = d_da;                       P.g_pre1 = P.g_r2 + rows * h->d;  P.g_z1 = P.g_pre1 + rows * h->d_inner;
    P.g_r1 = P.g_z1 + rows * h->d;       P.g_o = P.g_r1 + rows * h->d;     P.g_q = P.g_o + rows * h->d_v;
    P.g_preq = P.g_q + rows * h->d;
    P.gm = static_cast<float*>(d_work); P.dxr = P.gm + act; P.dstat = P.dxr + act;
    hipStream_t st = (hipStream_t)stream;
    const int tiles = P.TP >> 4;
    attn_bwd_row_kernel<<<B * tiles, 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    attn_bwd_stats_kernel<<<dim3(tiles, tiles), AT_STAT_WAVES * 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    attn_bwd_q_kernel<<<B * tiles, 64, 0, st>>>(P);
    HIP_TRY(hipGetLastError());
    if (d_gx) {
        attn_bwd_col_kernel<<<B * tiles, 64, 0, st>>>(P);
        HIP_TRY(hipGetLastError());
    }
    return DSP_OK;
}

}  // extern "C"

namespace {

int selfattn_pool(const char* who, const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                  const float* d_c, float* d_out, float* d_w, const int32_t* d_rows, void* stream) {
    if (!d_y || !d_W || !d_bW || !d_v || !d_c || !d_out) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (T < 1 || T > AT_MAX_T) return dsp_fail(DSP_EINVAL, "%s: T %d must be in [1, %d]", who, T, AT_MAX_T);
    if (B < 1) return dsp_fail(DSP_EINVAL, "%s: B %d must be >= 1", who, B);
    if (!mult4_in(H, AT_MAX_H)) return dsp_fail(DSP_EINVAL, "%s: H %d must be a multiple of 4 in [4, %d]", who, H, AT_MAX_H);
    if (((reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_W)) & 15) != 0)
        return dsp_fail(DSP_EINVAL, "%s: d_y and d_W must be 16-byte aligned", who);
    if (int rc = attn_check_launch(who, nullptr)) return rc;
    selfattn_pool_kernel<<<B, 64, 0, (hipStream_t)stream>>>(d_y, T, B, H, d_W, d_bW, d_v, d_c, d_out, d_w, d_rows);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_selfattn_pool_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                            const float* d_c, float* d_out, void* stream) {
    return selfattn_pool("dsp_selfattn_pool_batch", d_y, T, B, H, d_W, d_bW, d_v, d_c, d_out, nullptr, nullptr, stream);
}

int dsp_selfattn_pool_rows_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                 const float* d_c, float* d_out, const int32_t* d_rows, void* stream) {
    const char* who = "dsp_selfattn_pool_rows_batch";
    if (!d_rows) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    return selfattn_pool(who, d_y, T, B, H, d_W, d_bW, d_v, d_c, d_out, nullptr, d_rows, stream);
}

int dsp_selfattn_pool_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                  const float* d_c, float* d_out, float* d_w, void* stream) {
    const char* who = "dsp_selfattn_pool_train_batch";
    if (!d_w) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    return selfattn_pool(who, d_y, T, B, H, d_W, d_bW, d_v, d_c, d_out, d_w, nullptr, stream);
}

int dsp_selfattn_pool_rows_train_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW,
                                       const float* d_v, const float* d_c, float* d_out, float* d_w, const int32_t* d_rows, void* stream) {
    const char* who = "dsp_selfattn_pool_rows_train_batch";
    if (!d_w || !d_rows) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    return selfattn_pool(who, d_y, T, B, H, d_W, d_bW, d_v, d_c, d_out, d_w, d_rows, stream);
}

}  // extern "C"

namespace {

int selfattn_pool_backward(const char* who, const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW,
                           const float* d_v, const float* d_w, const float* d_gout, float* d_gy, float* d_gpre, float* d_ge, float* d_gvpart,
                           const int32_t* d_rows, void* stream) {
    if (!d_y || !d_W || !d_bW || !d_v || !d_w || !d_gout || !d_gpre || !d_ge || !d_gvpart) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    if (T < 1 || T > AT_MAX_T) return dsp_fail(DSP_EINVAL, "%s: T %d must be in [1, %d]", who, T, AT_MAX_T);
    if (B < 1) return dsp_fail(DSP_EINVAL, "%s: B %d must be >= 1", who, B);
    if (!mult4_in(H, AT_MAX_H)) return dsp_fail(DSP_EINVAL, "%s: H %d must be a multiple of 4 in [4, %d]", who, H, AT_MAX_H);
    if (((reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_W) | reinterpret_cast<uintptr_t>(d_gout)) & 15) != 0)
        return dsp_fail(DSP_EINVAL, "%s: d_y, d_W and d_gout must be 16-byte aligned", who);
    if (int rc = attn_check_launch(who, nullptr)) return rc;
    selfattn_pool_bwd_kernel<<<B, 64, 0, (hipStream_t)stream>>>(d_y, T, B, H, d_W, d_bW, d_v, d_w, d_gout, d_gy, d_gpre, d_ge, d_gvpart, d_rows);
    HIP_TRY(hipGetLastError());
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_selfattn_pool_backward_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW, const float* d_v,
                                     const float* d_w, const float* d_gout, float* d_gy, float* d_gpre, float* d_ge, float* d_gvpart,
                                     void* stream) {
    return selfattn_pool_backward("dsp_selfattn_pool_backward_batch", d_y, T, B, H, d_W, d_bW, d_v, d_w, d_gout, d_gy, d_gpre, d_ge, d_gvpart,
                                  nullptr, stream);
}

int dsp_selfattn_pool_rows_backward_batch(const float* d_y, int32_t T, int32_t B, int32_t H, const float* d_W, const float* d_bW,
                                          const float* d_v, const float* d_w, const float* d_gout, float* d_gy, float* d_gpre, float* d_ge,
                                          float* d_gvpart, const int32_t* d_rows, void* stream) {
    const char* who = "dsp_selfattn_pool_rows_backward_batch";
    if (!d_rows) return dsp_fail(DSP_EINVAL, "%s: NULL argument", who);
    return selfattn_pool_backward(who, d_y, T, B, H, d_W, d_bW, d_v, d_w, d_gout, d_gy, d_gpre, d_ge, d_gvpart, d_rows, stream);
}

}  // extern "C"
