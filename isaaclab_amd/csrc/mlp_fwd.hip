// First-layer forward of the PPO update with the activation fused: Y = ELU(X W^T + b), in-features K <= 256 (235 observations).
//
// In the update (rsl_rl PPO.update -> ActorCritic.actor / .critic forward, upstream rsl_rl/modules/actor_critic.py) this layer was a
// library GEMM (24576 x 235) . (235 x 1024) -- actor and critic first layers stacked -- followed by an ELU pass that reads and writes the
// 100 MB result once more: 111 us + 37 us per minibatch.  One launch here, 130 us (tools/fwd_bench.py; 22 vs 30 us at K = 48):
//   * a workgroup owns 128 output columns; each of its four multiplier waves keeps the W rows of ITS 32 columns in REGISTERS for the
//     whole launch (an operand of v_mfma_f32_32x32x2_f32: lane = column, NS k-steps = NS VGPRs), fetched once through LDS;
//   * it walks its share of the M samples in tiles of 32 rows, double-buffered in LDS and filled by LDS DMA (K > 128) or through
//     registers (K <= 128, where the registers are there);
//   * bias + ELU are applied to the accumulators and the activated tile is stored once -- for K > 128 by four helper waves of the
//     same workgroup, out of an LDS staging tile, while the multipliers run the next tile (k_mlp_fwd_elu_roles below).
// What bounds it (NOTES.md): the MFMA chain itself is 86 us (157 TFLOP/s fp32 peak -> 78 us).  In a four-wave workgroup each
// vector-memory instruction a wave issues between MFMAs (8 DMAs + 16 row stores per 120 MFMAs) cost it ~100 issue cycles that a second
// wave per SIMD did not hide: 141 us; with the helper waves issuing them 130 us (117.7 against 127.9 us inside the update).  What is left
// on top of the chain: launch + weights, and the helpers' bias + ELU arithmetic, whose VALU cycles come off the same SIMD's fp32 MFMA
// stream almost 1 : 1 (13 us of 113 us in a warm loop; 7 us of it the ELU).
// Exact fp32 products accumulated in fp32; the summation order differs from the library's (k and NS + k paired per step), tested against
// torch within the tolerance of the whole-update test.  PARITY UNPINNED like the rest of the rsl_rl restatement.
#include "imx_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int FW_KMAX = 256;          // in-features supported (k held in registers: FW_KMAX / 2 VGPRs per lane)
constexpr int FW_ROWS = 32;           // samples per tile
constexpr int FW_KP = FW_KMAX + 4;    // LDS row pitch in floats: rows stay 16-byte aligned and 8 consecutive rows cover the 32 banks with b128 reads
constexpr int FW_COLS = 128;          // output columns per workgroup (4 waves x 32)

__device__ __forceinline__ int acc_row32(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// Epilogue of one 32 x 32 accumulator tile: rows = samples on the accumulator registers, columns = out-features on the lanes.
// `y` points at this lane's column in the tile's first row of its half (row0 + 4 half); `rows` = rows of the tile that exist.
// Kept lean on purpose: the two workgroups of a CU fall into step (both in the MFMA phase, then both here), so every VALU
// instruction of the epilogue is time the MFMA pipe idles -- one 64-bit pointer walked by ldy, the ELU branch and the row guard hoisted.
template <bool ELU, bool FULL>
__device__ __forceinline__ void store_rows(const f32x16& acc, float bias, float alpha, float* y, int64_t ldy, int rows, int half) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float* yg = y + (int64_t)(8 * g) * ldy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = acc[4 * g + j] + bias;
            if (ELU) {
                const float e = (__expf(fminf(x, 0.0f)) - 1.0f) * alpha;
                x = x <= 0.0f ? e : x;
            }
            if (FULL || 8 * g + j + 4 * half < rows) yg[0] = x;
            yg += ldy;
        }
    }
}

__device__ __forceinline__ void store_tile(const f32x16& acc, float bias, float alpha, int elu, float* y, int64_t ldy, int rows, int half) {
    if (rows >= FW_ROWS) {
        if (elu) store_rows<true, true>(acc, bias, alpha, y, ldy, rows, half);
        else store_rows<false, true>(acc, bias, alpha, y, ldy, rows, half);
    } else {
        if (elu) store_rows<true, false>(acc, bias, alpha, y, ldy, rows, half);
        else store_rows<false, false>(acc, bias, alpha, y, ldy, rows, half);
    }
}

struct FwArgs {
    int64_t M;
    int N, K;
    const float* X;
    int64_t ldx;
    const float* W;   // (N, K) row-major, dense
    const float* b;   // (N)
    float* Y;
    int64_t ldy;
    float alpha;
    int ncb;          // column blocks = ceil(N / 128)
    int rs;           // row splits
    int64_t rps;      // rows per split (multiple of FW_ROWS)
    int elu;
};

// NS = MFMA steps per tile (each consumes two k): the k range [0, 2 NS) covers K; k >= K meets zero weights AND zero tile columns.
// MFMA step s pairs k = s (lanes 0..31) with k = NS + s (lanes 32..63): both operands are then CONTIGUOUS in s per lane, so the A operand
// comes out of LDS sixteen bytes (four steps) at a time and nothing in the step loop depends on K.
template <int NS, bool XVEC>
__global__ void __launch_bounds__(256, 2) k_mlp_fwd_elu(FwArgs a) {
    static_assert(NS % 4 == 0 && 2 * NS <= FW_KMAX, "step count");
    __shared__ __attribute__((aligned(16))) float sA[2][FW_ROWS * FW_KP];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, half = lane >> 5;
    const int cb = blockIdx.x % a.ncb, split = blockIdx.x / a.ncb;  // the column blocks of one row split run together: X tiles shared through L2
    const int col = cb * FW_COLS + w * 32 + r;
    const bool col_ok = col < a.N;
    const int K = a.K;
    // ---- this wave's weights: lane (column r, k-half `half`) holds W[col][half * NS + s], s = 0 .. NS
    float breg[NS];
    {
        const float* wr = a.W + (size_t)(col_ok ? col : a.N - 1) * K;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = half * NS + s;
            const float v = wr[k < K ? k : K - 1];  // (unconditional load, clamped: no branch per register)
            breg[s] = (k < K && col_ok) ? v : 0.0f;
        }
    }
    const float bias = col_ok ? a.b[col] : 0.0f;
    const int64_t m_begin = (int64_t)split * a.rps, m_end = min(m_begin + a.rps, a.M);
    const int ntile = (int)((m_end - m_begin + FW_ROWS - 1) / FW_ROWS);
    // ---- staging: 256 threads move one 32 x 2NS tile as float4; XVEC: 16-byte global loads (rows start on 16-byte boundaries), else 4-byte
    constexpr int C4 = 2 * NS / 4;                      // float4 per tile row
    constexpr int NV = (FW_ROWS * C4 + 255) / 256;      // float4 per thread per tile
    float4 pre[NV];
    auto g_load = [&](int tile) {
        const int64_t row0 = m_begin + (int64_t)tile * FW_ROWS;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / C4, c4 = idx - rr * C4;
            const int64_t row = min(row0 + rr, m_end - 1);      // (rows past the end are loaded again and never stored)
            const int k0 = 4 * c4;
            const float* p = a.X + row * a.ldx + (k0 < K ? k0 : 0);
            float4 v;
            if (XVEC) {
                v = *reinterpret_cast<const float4*>(p);
            } else {
                v.x = p[0];
                v.y = p[k0 + 1 < K ? 1 : 0];
                v.z = p[k0 + 2 < K ? 2 : 0];
                v.w = p[k0 + 3 < K ? 3 : 0];
            }
            // columns >= K (the pad of the row pitch, and the tail of the 2 NS range) must be ZERO in the tile: a NaN there would survive the zero weight
            v.x = k0 + 0 < K ? v.x : 0.f;
            v.y = k0 + 1 < K ? v.y : 0.f;
            v.z = k0 + 2 < K ? v.z : 0.f;
            v.w = k0 + 3 < K ? v.w : 0.f;
            pre[i] = v;
        }
    };
    auto s_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / C4, c4 = idx - rr * C4;
            if (FW_ROWS * C4 % 256 == 0 || rr < FW_ROWS) *reinterpret_cast<float4*>(sA[buf] + rr * FW_KP + 4 * c4) = pre[i];
        }
    };
    if (ntile > 0) {
        g_load(0);
        s_store(0);
    }
    __syncthreads();
    for (int tile = 0; tile < ntile; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntile) g_load(tile + 1);  // in flight during the MFMAs below
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        const float4* pa = reinterpret_cast<const float4*>(sA[buf] + r * FW_KP + half * NS);  // A operand: lane (row r, k-half) reads A[r][half NS + s]
#pragma unroll
        for (int s4 = 0; s4 < NS / 4; ++s4) {
            const float4 av = pa[s4];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, breg[4 * s4 + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, breg[4 * s4 + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, breg[4 * s4 + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, breg[4 * s4 + 3], acc, 0, 0, 0);
        }
        const int64_t row0 = m_begin + (int64_t)tile * FW_ROWS;
        if (col_ok) store_tile(acc, bias, a.alpha, a.elu, a.Y + (row0 + 4 * half) * a.ldy + col, a.ldy, (int)min<int64_t>(m_end - row0, FW_ROWS), half);
        if (tile + 1 < ntile) s_store(buf ^ 1);  // that buffer was last read in tile - 1: every wave is past the barrier below
        __syncthreads();
    }
}

// K > 128, 16-byte aligned rows (the XVEC condition): the same tile walk by a workgroup of EIGHT waves with two roles, one workgroup per CU.
//   * waves 0-3, the multipliers, run nothing but the MFMA stream out of LDS: no global load, no DMA, no global store.  The MFMA operands
//     are swapped against k_mlp_fwd_elu (A = weights, B = samples; the same products into the same accumulator in the same order), which
//     puts lane = sample row and four CONSECUTIVE out-features on each register group: after a tile's last MFMA the raw accumulators go
//     to an LDS staging tile (32 rows x 128 columns) as four 16-byte writes per lane;
//   * waves 4-7, the helpers, fill the next tile by LDS DMA (global_load_lds_dwordx4: no staging registers, no LDS write instructions;
//     one DMA per tile row, lane = float4 of the row -- the destination of a wave instruction is contiguous by lane, so a row pitch of
//     >= 1 KiB keeps rows apart), zero its columns >= K once they have landed (row-pitch pad / tail of the 2 NS range: a NaN there would
//     survive the zero weight) and run the epilogue of the PREVIOUS tile out of its staging tile: bias, ELU, one 16-byte store per lane
//     (512 contiguous bytes of a row per half wave).  Row and column predicates live here, where they cost the MFMA stream nothing.
// Tile buffers and staging tiles are double-buffered; one barrier per tile.
constexpr int FW_SP = FW_COLS + 4;    // staging row pitch in floats: 8 consecutive rows x 4 dwords cover the 32 banks of a 16-byte LDS write

template <int NS>
struct FwLds {                        // LDS map in floats
    static constexpr int TILE = FW_ROWS * FW_KP;
    static constexpr int STAGE = FW_ROWS * FW_SP;
    static constexpr int WBLK = FW_COLS * 2 * NS;                            // prologue: the W rows of the column block, dense (K <= 2 NS)
    static constexpr bool T0_FREE = (TILE + WBLK) * 4 <= 160 * 1024;         // room for tile 0 NEXT TO the weights: its DMA overlaps the prologue
    static constexpr int W_OFF = T0_FREE ? TILE : 0;
    static constexpr int LOOP = 2 * TILE + 2 * STAGE;                        // tile buffers, then staging tiles
    static constexpr int TOTAL = W_OFF + WBLK > LOOP ? W_OFF + WBLK : LOOP;
};

template <int NS>
__global__ void __launch_bounds__(512, 1) k_mlp_fwd_elu_roles(FwArgs a) {
    static_assert(NS % 8 == 0 && 2 * NS <= FW_KMAX, "step count");
    using L = FwLds<NS>;
    static_assert(L::TOTAL * 4 <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) float lds[L::TOTAL];
    float* const sA = lds;                 // [2][TILE]
    float* const sS = lds + 2 * L::TILE;   // [2][STAGE]
    float* const wl = lds + L::W_OFF;      // prologue only
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, r = lane & 31, half = lane >> 5;
    const bool helper = w >= 4;
    const int h = w & 3;
    // consecutive workgroup ids go to different XCDs (8, each with its own L2): renumber so that the column blocks of one row split --
    // which read the same X rows -- are neighbours on ONE XCD
    const int nb = gridDim.x, per = nb >> 3;
    const int vb = (nb & 7) == 0 ? (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int cb = vb % a.ncb, split = vb / a.ncb;
    const int K = a.K;
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&lds[0];
    const int64_t m_begin = (int64_t)split * a.rps, m_end = min(m_begin + a.rps, a.M);
    const int ntile = (int)((m_end - m_begin + FW_ROWS - 1) / FW_ROWS);
    // ---- helpers' tile fill: wave h moves rows 8 h .. 8 h + 7
    constexpr int C4 = 2 * NS / 4;  // float4 per tile row (<= 64 lanes)
    const int k0 = 4 * lane;
    const int64_t lane_off = (lane < C4 && k0 < K) ? k0 : 0;  // lanes past the row's data re-read its first vector (in bounds; zeroed below / never read)
    const int nz = 2 * NS - K;                                 // columns to zero per row
    auto dma_tile = [&](int tile, int buf) {
        const int64_t row0 = m_begin + (int64_t)tile * FW_ROWS + 8 * h;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t row = min(row0 + i, m_end - 1);  // (rows past the end: loaded again, never stored)
            const float* src = a.X + row * a.ldx + lane_off;
            // destination: wave-uniform LDS byte address in M0, the hardware adds lane * 16 bytes.  Inline asm rather than
            // __builtin_amdgcn_global_load_lds: after the builtin the compiler waits vmcnt(0) before the next LDS read (it cannot tell the
            // buffers apart), which would put the DMA latency in front of the epilogue's reads; the waits are explicit below.
            const unsigned dst = lds_base + (unsigned)((buf * FW_ROWS + 8 * h + i) * FW_KP * 4);
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst)) : "memory");
        }
    };
    const int zoff = lane < 8 * nz ? (8 * h + lane / nz) * FW_KP + K + lane % nz : -1;  // this lane's element of the first 64 (nz <= 8: all of them)
    auto zero_tail = [&](int buf) {
        float* tb = sA + buf * L::TILE;
        if (zoff >= 0) tb[zoff] = 0.0f;
        for (int i = lane + 64; i < 8 * nz; i += 64) {
            const int rr = i / nz, c = i - rr * nz;
            tb[(8 * h + rr) * FW_KP + K + c] = 0.0f;
        }
    };
    // ---- prologue.  The W rows of this column block are ONE contiguous run of 128 K floats.  Lane = column wants a row each, i.e. a
    // 4 K-byte stride between lanes: read that way every load instruction touches 64 cache lines (measured: ~50 us of a 160 us launch).
    // Instead the run comes through LDS, all four waves' blocks at once: read flat and coalesced by all eight waves, then every
    // multiplier lane picks its row.
    {
        const int64_t cb0 = (int64_t)cb * FW_COLS * K;                                          // flat offset of the run in W (a multiple of 128 floats)
        const int64_t avail = min<int64_t>((int64_t)FW_COLS * K, (int64_t)a.N * K - cb0);       // floats of it that exist (last column block); > 0
        const int64_t avail4 = avail & ~(int64_t)3;                                             // ... covered by whole, aligned float4
        const bool wdma = ((reinterpret_cast<uintptr_t>(a.W) & 15) == 0) && avail4 >= 4;
        if (wdma) {
            // flat and contiguous on both sides: exactly the shape of the LDS DMA (1 KiB per instruction, nothing staged in registers,
            // all of them in flight together -- a load/store loop pays one memory latency per iteration: ~20 us of the launch)
            for (int i = 256 * w; i < FW_COLS * K; i += 8 * 256) {   // (a last piece runs at most 128 floats past 128 K: inside WBLK, K < 2 NS then)
                const float* src = a.W + cb0 + min<int64_t>(i + 4 * lane, avail4 - 4);  // (past the run: re-read its last whole vector; those columns are masked)
                unsigned keep;
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_base + (unsigned)(L::W_OFF + i) * 4u)) : "memory");
            }
        } else {
            for (int i = 4 * t; i < FW_COLS * K; i += 4 * 512) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const float* src = a.W + cb0 + i;
                if (i + 0 < avail) v.x = src[0];
                if (i + 1 < avail) v.y = src[1];
                if (i + 2 < avail) v.z = src[2];
                if (i + 3 < avail) v.w = src[3];
                *reinterpret_cast<float4*>(wl + i) = v;
            }
        }
        if (L::T0_FREE && helper && ntile > 0) dma_tile(0, 0);  // the first tile travels with the weights
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (L::T0_FREE && helper && ntile > 0) zero_tail(0);
        __syncthreads();
        // a ragged last column block whose float count is not a multiple of four: its last 1-3 floats belong to a VALID column and sit
        // in a vector the clamp above replaced -- fetch them one by one, behind every wave's DMA
        if (wdma && t < avail - avail4) wl[avail4 + t] = a.W[cb0 + avail4 + t];
        __syncthreads();
    }
    if (!helper) {
        // ------------------------------------------------------------------------------------------------ multipliers
        const int col = cb * FW_COLS + w * 32 + r;
        const bool col_ok = col < a.N;
        // this wave's weights: lane (column r, k-half `half`) holds W[col][half * NS + s], s = 0 .. NS
        float breg[NS];
        {
            const float* wrow = wl + (w * 32 + r) * K + half * NS;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = half * NS + s;
                const float v = wrow[k < K ? s : 0];  // (unconditional, clamped: the reads pipeline)
                breg[s] = (k < K && col_ok) ? v : 0.0f;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (!L::T0_FREE) __syncthreads();  // the first tile lands on top of the weights' staging area
        __syncthreads();                   // tile 0 is in LDS; the staging area is free
        for (int tile = 0; tile < ntile; ++tile) {
            const int buf = tile & 1;
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
            // B operand: lane (sample row r, k-half) reads X[r][half NS + s]; step s pairs k = s with k = NS + s
            const float4* pa = reinterpret_cast<const float4*>(sA + buf * L::TILE + r * FW_KP + half * NS);
            // Operand ping-pong: the LDS reads of the next eight steps are issued BEFORE the eight MFMAs of these and waited for after
            // them (this wave is the only multiplier of its SIMD: nobody else fills a read's latency); the scheduling barriers keep the
            // compiler from sinking the reads behind the MFMAs again.
            float4 op[2][2];
            op[0][0] = pa[0];
            op[0][1] = pa[1];
#pragma unroll
            for (int c = 0; c < NS / 8; ++c) {
                if (c + 1 < NS / 8) {
                    op[(c + 1) & 1][0] = pa[2 * c + 2];
                    op[(c + 1) & 1][1] = pa[2 * c + 3];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float4 av = op[c & 1][j];
                    const int s = 8 * c + 4 * j;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(breg[s + 0], av.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(breg[s + 1], av.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(breg[s + 2], av.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(breg[s + 3], av.w, acc, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // accumulator register 4 g + j of lane (sample r, half) is out-feature 8 g + 4 half + j of this wave's 32
            float* ps = sS + buf * L::STAGE + r * FW_SP + w * 32 + 4 * half;
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(ps + 8 * g) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // that staging tile is next written in tile + 2: the helpers have read it before the barrier in between
        }
        return;
    }
    // ---------------------------------------------------------------------------------------------------- helpers
    const int c4 = lane & 31, rsub = lane >> 5;   // a half wave per staging row, a lane per float4 of it
    const int colh = cb * FW_COLS + 4 * c4;
    float4 b4;
    b4.x = colh + 0 < a.N ? a.b[colh + 0] : 0.0f;
    b4.y = colh + 1 < a.N ? a.b[colh + 1] : 0.0f;
    b4.z = colh + 2 < a.N ? a.b[colh + 2] : 0.0f;
    b4.w = colh + 3 < a.N ? a.b[colh + 3] : 0.0f;
    const bool yvec = ((reinterpret_cast<uintptr_t>(a.Y) & 15) == 0) && (a.ldy & 3) == 0;  // (colh is a multiple of four)
    const bool wide = yvec && (cb + 1) * FW_COLS <= a.N;                                    // every lane stores sixteen bytes: workgroup-uniform
    const float alpha = a.alpha;
    const int elu = a.elu;
    auto act = [&](float x) {
        const float e = (__expf(fminf(x, 0.0f)) - 1.0f) * alpha;
        return x <= 0.0f ? e : x;
    };
    // epilogue of one tile out of its staging tile: wave h takes rows 8 h .. 8 h + 7, two per instruction
    auto epilogue = [&](int tile, bool full) {
        const int64_t row0 = m_begin + (int64_t)tile * FW_ROWS;
        const int rows = full ? FW_ROWS : (int)min<int64_t>(m_end - row0, FW_ROWS);
        const float* ps = sS + (tile & 1) * L::STAGE + (8 * h + rsub) * FW_SP + 4 * c4;
        float* y = a.Y + (row0 + 8 * h + rsub) * a.ldy + colh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 v = *reinterpret_cast<const float4*>(ps + 2 * i * FW_SP);
            v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
            if (elu) { v.x = act(v.x); v.y = act(v.y); v.z = act(v.z); v.w = act(v.w); }
            float* yr = y + (int64_t)(2 * i) * a.ldy;
            if (wide) {
                if (full || 8 * h + rsub + 2 * i < rows) *reinterpret_cast<f32x4*>(yr) = f32x4{v.x, v.y, v.z, v.w};  // (one vector store: as a float4 struct its last element is merged with the branch below)
            } else if (8 * h + rsub + 2 * i < rows) {
                if (colh + 0 < a.N) yr[0] = v.x;
                if (colh + 1 < a.N) yr[1] = v.y;
                if (colh + 2 < a.N) yr[2] = v.z;
                if (colh + 3 < a.N) yr[3] = v.w;
            }
        }
    };
    if (!L::T0_FREE) {
        __syncthreads();  // the multipliers have picked their weights out of the staging area
        if (ntile > 0) {
            dma_tile(0, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            zero_tail(0);
        }
    }
    __syncthreads();
    for (int tile = 0; tile < ntile; ++tile) {
        const bool more = tile + 1 < ntile;
        if (more) dma_tile(tile + 1, (tile & 1) ^ 1);  // that buffer was last read in tile - 1: every multiplier is past its barrier
        if (tile > 0) epilogue(tile - 1, true);         // (every tile but the last is full)
        // Wait for the DMAs only.  A store is acknowledged microseconds later under load and need not be waited for: the counter
        // retires in issue order, so "at most the four youngest outstanding" says the DMAs issued before the four stores have landed.
        if (tile > 0 && wide) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (more) zero_tail((tile & 1) ^ 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // (raw: a __syncthreads() here would also wait for the stores)
    }
    if (ntile > 0) epilogue(ntile - 1, false);
}

template <bool XVEC>
void launch_fwd(const FwArgs& a, dim3 grid, hipStream_t st) {
    const int ns = (a.K + 1) / 2;
    if (XVEC && ns > 64) {  // the eight-wave kernel: the weights of 2 NS in-features need the LDS DMA to fit the registers
        const dim3 block(512);
        if (ns <= 96) hipLaunchKernelGGL((k_mlp_fwd_elu_roles<96>), grid, block, 0, st, a);
        else if (ns <= 120) hipLaunchKernelGGL((k_mlp_fwd_elu_roles<120>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mlp_fwd_elu_roles<128>), grid, block, 0, st, a);
        return;
    }
    const dim3 block(256);
    if (ns <= 32) hipLaunchKernelGGL((k_mlp_fwd_elu<32, XVEC>), grid, block, 0, st, a);
    else if (ns <= 64) hipLaunchKernelGGL((k_mlp_fwd_elu<64, XVEC>), grid, block, 0, st, a);
    else if (ns <= 96) hipLaunchKernelGGL((k_mlp_fwd_elu<96, false>), grid, block, 0, st, a);  // unaligned rows: staged through registers (spills above 96 steps)
    else if (ns <= 120) hipLaunchKernelGGL((k_mlp_fwd_elu<120, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_mlp_fwd_elu<128, false>), grid, block, 0, st, a);
}

}  // namespace

extern "C" int imx_mlp_fwd_elu(int64_t M, int N, int K, const float* X_d, int64_t ldx, const float* W_d, const float* b_d, float elu_alpha,
                               int apply_elu, float* Y_d, int64_t ldy, imx_stream_t stream) {
    IMX_REQUIRE(M > 0 && N > 0 && K > 0 && X_d && W_d && b_d && Y_d, "imx_mlp_fwd_elu: bad arguments");
    IMX_REQUIRE(K <= FW_KMAX, "imx_mlp_fwd_elu: %d in-features (at most %d: the weights of a column live in registers)", K, FW_KMAX);
    IMX_REQUIRE(ldx >= K && ldy >= N, "imx_mlp_fwd_elu: row pitch smaller than the row");
    static int num_cu = 0;
    if (num_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || num_cu <= 0)
            num_cu = 256;
    }
    FwArgs a;
    a.M = M; a.N = N; a.K = K; a.X = X_d; a.ldx = ldx; a.W = W_d; a.b = b_d; a.Y = Y_d; a.ldy = ldy; a.alpha = elu_alpha; a.elu = apply_elu;
    a.ncb = (N + FW_COLS - 1) / FW_COLS;
    const bool xvec = (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(X_d) & 15) == 0) && (K % 4 == 0 || ldx >= ((K + 3) & ~3));
    // four-wave kernels: two workgroups per CU (LDS 66 KB each, <= 256 VGPRs); the eight-wave kernel: one.  Row splits so that the grid
    // is that many times #CU workgroups, each >= 4 tiles
    const int wg_per_cu = (xvec && (K + 1) / 2 > 64) ? 1 : 2;
    int64_t rs = std::max<int64_t>(1, (wg_per_cu * (int64_t)num_cu) / a.ncb);
    rs = std::min<int64_t>(rs, std::max<int64_t>(1, M / (4 * FW_ROWS)));
    a.rps = ((M + rs - 1) / rs + FW_ROWS - 1) / FW_ROWS * FW_ROWS;
    a.rs = (int)((M + a.rps - 1) / a.rps);
    const dim3 grid((unsigned)(a.ncb * a.rs));
    if (xvec) launch_fwd<true>(a, grid, (hipStream_t)stream);
    else launch_fwd<false>(a, grid, (hipStream_t)stream);
    IMX_HIP(hipGetLastError());
    return 0;
}
