// The MFMA inference layers and the loop over them (infer_layers, at the end), shared by the rollout inference kernels (mlp.hip) and the
// fused low-level policy step (pretrained_policy.hip) ("Low-level policy step").
#pragma once

#include "imx_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// row of a 32x32 MFMA accumulator register: lanes 0-31 hold rows {0-3, 8-11, 16-19, 24-27}, lanes 32-63 the others
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

constexpr int INF_ROWS = 32, INF_MAXD = 512, INF_PITCH = INF_MAXD + 4, INF_MAXL = 4;

// One layer for the 32 samples of the workgroup.  NBW = 32-column output blocks per wave (4, 2 or 1); a reduction GROUP is
// GS = 4 / NBW sub-groups of 32 indices, so that every group is 64 MFMAs per wave (4096 cycles, more than an L2 round trip)
// whatever the layer width.  Two operand sets (P, Q) ping-pong: the loads of group g+1 are issued before the MFMAs of group
// g.  Every load in the loop is UNCONDITIONAL (indices clamped; the host guarantees zero-padded weight rows with a pitch
// that is a multiple of 32, activation columns beyond K are zero in LDS, column blocks beyond N re-read row N-1 and are
// dropped in the epilogue): a load inside a divergent branch makes the compiler wait for all outstanding loads at the
// join, which measured 2x slower here.
// PACKED: W points at the packed copy (imx_mlp_pack_weights): chunk ((cb * nsub + sc) * 4 + i) holds, lane by lane, exactly the float4
// the row layout's load (column block cb, sub-group sc, piece i) gives each lane -- one contiguous KiB per wave instruction instead of
// 32 rows x 2 x 16 bytes.  Lanes reading 32 different weight rows is what held this kernel at ~4 TB/s of L2 traffic (256 workgroups x
// 1.1 MB of weights per launch); contiguous pieces stream from L2 at several times that.
template <int NBW, bool PACKED>
__device__ __forceinline__ void infer_layer(const float* __restrict__ sIn, int K, const float* __restrict__ W, int ldw,
                                            const float* __restrict__ bias, int N, bool elu, float alpha, float* __restrict__ sOut,
                                            float* __restrict__ gOut, int64_t m0, int64_t M) {
    constexpr int GS = 4 / NBW;
    if ((int)(threadIdx.x >> 6) * 32 >= ((N + 31) & ~31)) return;  // this wave owns no column block of a narrow layer (the action head): wave-uniform
    // (Eight waves per workgroup -- two per SIMD splitting the column blocks, so that one multiplies while the other waits for weight rows --
    //  were measured: 106.8 us against 68.2 us for both networks at 4096 samples, the same 49 us for one network on half the chip.  What
    //  slows the launch down when all 256 CUs run it is the shared weight stream out of L2, not exposed latency inside a SIMD.)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, half = lane >> 5;
    f32x16 acc[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.0f;
    const int nsub = (K + 31) >> 5;            // 32-index sub-groups
    const int ng = (nsub + GS - 1) / GS;       // groups
    const float* wrow[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        if (PACKED) {
            const int ncb = (N + 31) >> 5, cb = w + 4 * j;
            wrow[j] = W + ((size_t)(cb < ncb ? cb : ncb - 1) * nsub * 4) * 256 + 4 * lane;  // (blocks past N re-read the last one; dropped below)
        } else {
            const int n = (w + 4 * j) * 32 + r;
            wrow[j] = W + (size_t)(n < N ? n : N - 1) * ldw + 16 * half;
        }
    }
    constexpr int WSTEP_SC = PACKED ? 4 * 256 : 32, WSTEP_I = PACKED ? 256 : 4;  // floats between sub-groups / between the four pieces
    const float* arow = sIn + r * INF_PITCH + 16 * half;
    float4 Pa[GS][4], Qa[GS][4], Pb[NBW][GS][4], Qb[NBW][GS][4];
    // sub-groups past the end (a group may be partial) are clamped to the last one for the loads and multiplied by zero
    auto load = [&](float4 (&a)[GS][4], float4 (&b)[NBW][GS][4], int g) {
#pragma unroll
        for (int u = 0; u < GS; ++u) {
            const int sg = g * GS + u;
            const int sc = sg < nsub ? sg : nsub - 1;
#pragma unroll
            for (int j = 0; j < NBW; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) b[j][u][i] = *reinterpret_cast<const float4*>(wrow[j] + WSTEP_SC * sc + WSTEP_I * i);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 v = *reinterpret_cast<const float4*>(arow + 32 * sc + 4 * i);
                if (sg >= nsub) v = make_float4(0.f, 0.f, 0.f, 0.f);
                a[u][i] = v;
            }
        }
    };
    auto mult = [&](const float4 (&a)[GS][4], const float4 (&b)[NBW][GS][4]) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < GS; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i].x, b[j][u][i].x, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i].y, b[j][u][i].y, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i].z, b[j][u][i].z, acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NBW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i].w, b[j][u][i].w, acc[j], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    load(Pa, Pb, 0);
    int g = 0;
    for (; g + 1 < ng; g += 2) {
        load(Qa, Qb, g + 1);
        mult(Pa, Pb);
        load(Pa, Pb, g + 2 < ng ? g + 2 : ng - 1);  // clamped: at most one redundant reload at the end
        mult(Qa, Qb);
    }
    if (g < ng) mult(Pa, Pb);  // odd number of groups: P holds the last one
    // epilogue: accumulator rows = samples (registers), columns = out-features (lanes).  Branch-free arithmetic (ELU as a
    // select over an unconditionally evaluated exp) and unconditional LDS stores: a store inside a divergent branch makes
    // the compiler wait for the previous one.  Columns beyond N of a hidden layer land in the zero-padding region, which
    // is re-zeroed by the caller before the next layer reads it -- only the last layer (global stores) is guarded.
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const int n = (w + 4 * j) * 32 + r;
        const float bv = bias[n < N ? n : N - 1];
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float x = acc[j][q] + bv;
            const float e = (expf(fminf(x, 0.0f)) - 1.0f) * alpha;
            v[q] = (elu && x <= 0.0f) ? e : x;
        }
        if (sOut) {
            if (n < INF_MAXD) {
#pragma unroll
                for (int q = 0; q < 16; ++q) sOut[acc_row(q, half) * INF_PITCH + n] = n < N ? v[q] : 0.0f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = acc_row(q, half);
                if (n < N && m0 + row < M) gOut[(m0 + row) * (int64_t)N + n] = v[q];
            }
        }
    }
}

// ---- 16-sample variant (v_mfma_f32_16x16x4_f32) for small batches: twice the workgroups (and half the LDS each) when
// 32-sample tiles would leave half of the CUs idle (<= 2048 envs for two networks on 256 CUs).  Same structure as above:
// NBW = 16-column blocks per wave (8, 4, 2, 1), a sub-group is 32 reduction indices = 8 MFMA steps per block (lane quarter
// kq supplies k = 32s + 4kq + {0..3} and 32s + 16 + 4kq + {0..3}: the four quarters cover one 128-byte weight line).
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int INF16_ROWS = 16;

template <int NBW>
__device__ __forceinline__ void infer_layer16(const float* __restrict__ sIn, int K, const float* __restrict__ W, int ldw,
                                              const float* __restrict__ bias, int N, bool elu, float alpha, float* __restrict__ sOut,
                                              float* __restrict__ gOut, int64_t m0, int64_t M) {
    constexpr int GS = NBW >= 8 ? 1 : (NBW == 4 ? 2 : 4);  // sub-groups per group: >= 64 MFMAs (2048 cycles) per group
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    f32x4 acc[NBW];
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[b][q] = 0.0f;
    const int nsub = (K + 31) >> 5;
    const int ng = (nsub + GS - 1) / GS;
    const float* wrow[NBW];
#pragma unroll
    for (int b = 0; b < NBW; ++b) {
        const int n = (w + 4 * b) * 16 + j;
        wrow[b] = W + (size_t)(n < N ? n : N - 1) * ldw + 4 * kq;
    }
    const float* arow = sIn + j * INF_PITCH + 4 * kq;
    float4 Pa[GS][2], Qa[GS][2], Pb[NBW][GS][2], Qb[NBW][GS][2];
    auto load = [&](float4 (&a)[GS][2], float4 (&bq)[NBW][GS][2], int g) {
#pragma unroll
        for (int u = 0; u < GS; ++u) {
            const int sg = g * GS + u;
            const int sc = sg < nsub ? sg : nsub - 1;
#pragma unroll
            for (int b = 0; b < NBW; ++b) {
                bq[b][u][0] = *reinterpret_cast<const float4*>(wrow[b] + 32 * sc);
                bq[b][u][1] = *reinterpret_cast<const float4*>(wrow[b] + 32 * sc + 16);
            }
            float4 v0 = *reinterpret_cast<const float4*>(arow + 32 * sc);
            float4 v1 = *reinterpret_cast<const float4*>(arow + 32 * sc + 16);
            if (sg >= nsub) { v0 = make_float4(0.f, 0.f, 0.f, 0.f); v1 = v0; }
            a[u][0] = v0;
            a[u][1] = v1;
        }
    };
    auto mult = [&](const float4 (&a)[GS][2], const float4 (&bq)[NBW][GS][2]) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < GS; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i].x, bq[b][u][i].x, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i].y, bq[b][u][i].y, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i].z, bq[b][u][i].z, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i].w, bq[b][u][i].w, acc[b], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    load(Pa, Pb, 0);
    int g = 0;
    for (; g + 1 < ng; g += 2) {
        load(Qa, Qb, g + 1);
        mult(Pa, Pb);
        load(Pa, Pb, g + 2 < ng ? g + 2 : ng - 1);
        mult(Qa, Qb);
    }
    if (g < ng) mult(Pa, Pb);
    // epilogue: 16x16 accumulator: column = lane & 15, row = (lane >> 4) * 4 + register (branch-free, as in infer_layer)
#pragma unroll
    for (int b = 0; b < NBW; ++b) {
        const int n = (w + 4 * b) * 16 + j;
        const float bv = bias[n < N ? n : N - 1];
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = acc[b][q] + bv;
            const float e = (expf(fminf(x, 0.0f)) - 1.0f) * alpha;
            v[q] = (elu && x <= 0.0f) ? e : x;
        }
        if (sOut) {
            if (n < INF_MAXD) {
#pragma unroll
                for (int q = 0; q < 4; ++q) sOut[(kq * 4 + q) * INF_PITCH + n] = n < N ? v[q] : 0.0f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = kq * 4 + q;
                if (n < N && m0 + row < M) gOut[(m0 + row) * (int64_t)N + n] = v[q];
            }
        }
    }
}

// The layers of one tile of ROWS (16 or 32) samples: what the rollout inference kernels and k_pretrained_policy do between their input
// tile and their epilogue.  The activations ping-pong between the LDS buffers `in` and `out`; per layer: zero the padding columns the
// next layer's 32-wide reduction groups will read, pick the column blocks per wave, run the layer, barrier, swap.  Returns the pair after
// the last swap: `in` is the buffer the last layer wrote (if it wrote to LDS), `out` the other one.
//   net       a struct with nlayers, dim[], ldw[], b[], alpha (InferNet, PolicyArgs)
//   W         the row layouts, or for <32, true> the packed images
//   last_to_lds / gout()   the last layer's output stays in LDS, or goes to the global rows gout() ((M, dim[nlayers]), rows past M dropped)
// How the arguments are passed is part of the kernels' register figures (NOTES.md, "One tile body for the inference kernels"): the
// buffers by value and returned (as float*& every caller's allocation moved), the global output as a callable read at each dispatch
// (as a float* read once before the loop, all 18 inference kernels moved).
struct InferBufs {
    float *in, *out;
};
template <int ROWS, bool PACKED, class Net, class GOut>
__device__ __forceinline__ InferBufs infer_layers(float* in, float* out, const Net& net, const float* const* W, bool last_to_lds, GOut gout,
                                                  int64_t m0, int64_t M) {
    static_assert(ROWS == INF_ROWS || (ROWS == INF16_ROWS && !PACKED), "16- or 32-row tiles; only the 32-row layer reads packed weights");
    for (int l = 0; l < net.nlayers; ++l) {
        const int K = net.dim[l], N = net.dim[l + 1];
        const bool last = l == net.nlayers - 1;
        float* so = (last && !last_to_lds) ? nullptr : out;
        if (!last) {
            const int Np = (N + 31) & ~31;
            for (int i = threadIdx.x; i < ROWS * (Np - N); i += blockDim.x) {
                const int row = i / (Np - N), col = N + i - row * (Np - N);
                out[row * INF_PITCH + col] = 0.0f;
            }
        }
        if constexpr (ROWS == INF16_ROWS) {
            const int nbw = ((N + 15) / 16 + 3) / 4;  // 16-column blocks per wave
            if (nbw <= 1) infer_layer16<1>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
            else if (nbw == 2) infer_layer16<2>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
            else if (nbw <= 4) infer_layer16<4>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
            else infer_layer16<8>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
        } else {
            const int nbw = ((N + 31) / 32 + 3) / 4;  // 32-column blocks per wave
            if (nbw <= 1) infer_layer<1, PACKED>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
            else if (nbw == 2) infer_layer<2, PACKED>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
            else infer_layer<4, PACKED>(in, K, W[l], net.ldw[l], net.b[l], N, !last, net.alpha, so, gout(), m0, M);
        }
        __syncthreads();
        float* t = in; in = out; out = t;
    }
    return {in, out};
}
