// Device-resident Adam (include/dsp_frontend.h: dsp_adam_*): a multi-tensor fp32 update, weight_decay = 0, amsgrad off, in two
// launches per step -- a one-thread prologue that advances the step count and derives the step's scalars in fp64, and one
// streaming launch over a chunk table.  Everything a step reads (pointer tables, hyper-parameters, step count, chunk table)
// lies in device memory, so a recorded step follows set_lr / set_step / bind without a re-capture.  No atomics, no LDS, no
// memset; every element is read and written by exactly one lane: the same bits on every run.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ADAM_CHUNK 1024      // elements of one chunk: one 16-byte access per lane and array
#define ADAM_THREADS 256
#define ADAM_BIND_BATCH 32   // gradient pointers one adam_bind_kernel launch carries as kernel arguments

// The optimiser's state in device memory.  The fp64 half is what the host sets; the fp32 half is what adam_advance_kernel
// derives from it for the step that follows.
struct AdamState {
    long long step;                       // steps taken so far
    double lr, beta1, beta2, eps;
    float b1, b2, omb1, omb2;             // beta1, beta2, 1 - beta1, 1 - beta2 (the differences formed in fp64)
    float step_size, bc2_sqrt, eps_f;     // lr / (1 - beta1^t), sqrt(1 - beta2^t), eps
    float reserved;
};

// One handle's tables, all in ONE device allocation behind `state`.
struct AdamTables {
    AdamState* state;
    float* const* p;                      // [n]
    float* const* m;                      // [n]
    float* const* v;                      // [n]
    float* const* g;                      // [n], written by adam_bind_kernel
    const int64_t* numel;                 // [n]
    const int64_t* chunk_off;             // [n_chunks] first element of the chunk inside its tensor, a multiple of ADAM_CHUNK
    const int32_t* chunk_tensor;          // [n_chunks]
    int64_t n_chunks;
};

struct AdamPtrBatch {
    float* ptr[ADAM_BIND_BATCH];
};

__global__ void adam_set_hyper_kernel(AdamState* s, double lr, double beta1, double beta2, double eps) {
    s->lr = lr;
    s->beta1 = beta1;
    s->beta2 = beta2;
    s->eps = eps;
}

__global__ void adam_set_step_kernel(AdamState* s, long long step) { s->step = step; }

__global__ void adam_bind_kernel(float** table, AdamPtrBatch batch, int32_t first, int32_t count) {
    const int32_t i = threadIdx.x;
    if (i < count) table[first + i] = batch.ptr[i];
}

// <<<1, 1>>> in front of every adam_step_kernel: the one place the step count moves, so that no workgroup of the update can
// race it and all of them read the same t.
__global__ void adam_advance_kernel(AdamState* s) {
    const long long t = s->step + 1;
    s->step = t;
    const double b1 = s->beta1, b2 = s->beta2;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    s->b1 = (float)b1;
    s->b2 = (float)b2;
    s->omb1 = (float)(1.0 - b1);
    s->omb2 = (float)(1.0 - b2);
    s->step_size = (float)(s->lr / bc1);
    s->bc2_sqrt = (float)sqrt(bc2);
    s->eps_f = (float)s->eps;
}

struct AdamCoef {
    float b1, b2, omb1, omb2, step_size, bc2_sqrt, eps;
};

// One element.  Every rounding is spelled out (fmaf / a product / a quotient), so that the 16-byte and the scalar route give
// the same bits whatever the compiler would contract.
__device__ __forceinline__ void adam_element(const AdamCoef& c, float g, float& p, float& m, float& v) {
    m = fmaf(c.b1, m, c.omb1 * g);
    v = fmaf(c.b2, v, (c.omb2 * g) * g);
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), c.bc2_sqrt), c.eps);
    p = fmaf(-c.step_size, __fdiv_rn(m, denom), p);
}

// A workgroup grid-strides over chunks; the descriptor of a chunk and its tensor's pointers are wave-uniform reads.  ZERO:
// write 0.0f over each gradient after reading it (zero_grad(set_to_none=False) fused).
template <bool ZERO>
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(AdamTables tb) {
    const AdamState* s = tb.state;
    const AdamCoef c = {s->b1, s->b2, s->omb1, s->omb2, s->step_size, s->bc2_sqrt, s->eps_f};
    for (int64_t ch = blockIdx.x; ch < tb.n_chunks; ch += gridDim.x) {
        const int32_t t = tb.chunk_tensor[ch];
        const int64_t off = tb.chunk_off[ch];
        const int64_t left = tb.numel[t] - off;
        const int32_t cnt = left < ADAM_CHUNK ? (int32_t)left : ADAM_CHUNK;
        float* __restrict__ p = tb.p[t] + off;
        float* __restrict__ m = tb.m[t] + off;
        float* __restrict__ v = tb.v[t] + off;
        float* __restrict__ g = tb.g[t] + off;
        // off is a multiple of 4 elements: the chunk is aligned where the tensor is
        const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                            reinterpret_cast<uintptr_t>(g)) & 15) == 0;
        const int32_t nvec = wide ? cnt >> 2 : 0;
        for (int32_t i = threadIdx.x; i < nvec; i += ADAM_THREADS) {
            const float4 g4 = reinterpret_cast<const float4*>(g)[i];
            float4 p4 = reinterpret_cast<const float4*>(p)[i];
            float4 m4 = reinterpret_cast<const float4*>(m)[i];
            float4 v4 = reinterpret_cast<const float4*>(v)[i];
            adam_element(c, g4.x, p4.x, m4.x, v4.x);
            adam_element(c, g4.y, p4.y, m4.y, v4.y);
            adam_element(c, g4.z, p4.z, m4.z, v4.z);
            adam_element(c, g4.w, p4.w, m4.w, v4.w);
            reinterpret_cast<float4*>(p)[i] = p4;
            reinterpret_cast<float4*>(m)[i] = m4;
            reinterpret_cast<float4*>(v)[i] = v4;
            if (ZERO) reinterpret_cast<float4*>(g)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        // a misaligned tensor, and the numel % 4 tail of an aligned one
        for (int32_t i = nvec * 4 + threadIdx.x; i < cnt; i += ADAM_THREADS) {
            const float gi = g[i];
            float pi = p[i], mi = m[i], vi = v[i];
            adam_element(c, gi, pi, mi, vi);
            p[i] = pi;
            m[i] = mi;
            v[i] = vi;
            if (ZERO) g[i] = 0.0f;
        }
    }
}
