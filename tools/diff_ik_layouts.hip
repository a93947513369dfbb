// Measurement (DESIGN.md "Differential IK"): the two ways a lane can get its 6 x ND Jacobian block, timed under HIP events.
//   per-lane  each lane loads its own block straight from global memory (what k_diff_ik in csrc/diff_ik.hip does);
//   staged    the wave copies its 64 blocks through LDS with coalesced loads (consecutive lanes, consecutive floats) into rows of an
//             odd pitch, then every lane reads its own row.
// Both run diff_ik_env (csrc/imx_diff_ik.h) and must give the same bits.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/diff_ik_layouts.hip -o diff_ik_layouts
//   diff_ik_layouts [num_envs = 4096]
// Franka shapes: NB = 10, ND = 9, 7 joints, pose / relative / dls with the hand offset.  Per mode (1, 2, 3) and layout: the mean time
// of 2000 back-to-back launches, five alternating rounds, median and spread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../isaaclab_amd/csrc/imx_diff_ik.h"

#define WAVE 64
#define CHECK(e)                                                                        \
    do {                                                                                \
        hipError_t _s = (e);                                                            \
        if (_s != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(_s), __LINE__); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

__global__ void __launch_bounds__(WAVE) k_per_lane(imx_diff_ik_t c, int64_t N, int mode, DiffIkIO io) {
    const int64_t e = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (e >= N) return;
    diff_ik_env(c, e, mode, io, (mode & 2) ? io.jacobians + (e * io.NB + c.jacobi_body_idx) * 6 * io.ND : nullptr);
}

__global__ void __launch_bounds__(WAVE) k_staged(imx_diff_ik_t c, int64_t N, int mode, DiffIkIO io) {
    extern __shared__ float rows[];  // WAVE rows of pitch (6 ND) | 1 floats
    const int64_t e0 = (int64_t)blockIdx.x * WAVE, e = e0 + threadIdx.x;
    const int RW = 6 * (int)io.ND, pitch = RW | 1;
    if (mode & 2) {
        const int live = (int)(N - e0 < WAVE ? N - e0 : WAVE);
        for (int idx = threadIdx.x; idx < live * RW; idx += WAVE) {
            const int r = idx / RW, k = idx - r * RW;
            rows[r * pitch + k] = io.jacobians[((e0 + r) * io.NB + c.jacobi_body_idx) * RW + k];
        }
        __syncthreads();
    }
    if (e >= N) return;
    diff_ik_env(c, e, mode, io, rows + threadIdx.x * pitch);
}

int main(int argc, char** argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 4096;
    const int64_t B = 11, NB = 10, ND = 9, J = 9, PA = 6;
    if (N <= 0 || N > (1 << 20)) return 2;
    imx_diff_ik_t c;
    memset(&c, 0, sizeof c);
    c.command_type = IMX_IK_POSE; c.use_relative_mode = 1; c.ik_method = IMX_IK_DLS; c.has_offset = 1;
    c.lambda_val = 0.01f; c.k_val = 1.0f; c.offset_pos[2] = 0.107f; c.offset_rot[0] = 1.0f;
    c.body_idx = 8; c.jacobi_body_idx = 7; c.num_joints = 7;
    for (int j = 0; j < 7; ++j) c.joint_ids[j] = c.jacobi_joint_ids[j] = j;
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
    auto dev = [&](size_t n, float** p) -> hipError_t {
        std::vector<float> h(n);
        for (auto& x : h) x = rnd();
        hipError_t st = hipMalloc(p, n * 4);
        return st != hipSuccess ? st : hipMemcpy(*p, h.data(), n * 4, hipMemcpyHostToDevice);
    };
    float *act, *rp, *rq, *bp, *bq, *jac, *jp, *pd[2], *qd[2], *jd[2];
    CHECK(dev(N * PA, &act)); CHECK(dev(N * 3, &rp)); CHECK(dev(N * 4, &rq)); CHECK(dev(N * B * 3, &bp)); CHECK(dev(N * B * 4, &bq));
    CHECK(dev(N * NB * 6 * ND, &jac)); CHECK(dev(N * J, &jp));
    for (int v = 0; v < 2; ++v) {
        CHECK(hipMalloc(&pd[v], N * 3 * 4)); CHECK(hipMalloc(&qd[v], N * 4 * 4)); CHECK(hipMalloc(&jd[v], N * 7 * 4));
        CHECK(hipMemset(jd[v], 0, N * 7 * 4));
    }
    DiffIkIO io[2];
    for (int v = 0; v < 2; ++v) io[v] = DiffIkIO{act, PA, rp, rq, bp, bq, B, jac, NB, ND, jp, J, pd[v], qd[v], jd[v], 7};
    if (const char* why = imx_diff_ik_check(&c, N, 3, io[0])) {
        fprintf(stderr, "refused: %s\n", why);
        return 2;
    }
    const dim3 grid((unsigned)((N + WAVE - 1) / WAVE)), block(WAVE);
    const size_t lds = WAVE * ((6 * ND) | 1) * sizeof(float);
    auto launch = [&](int v, int mode) {
        if (v == 0) hipLaunchKernelGGL(k_per_lane, grid, block, 0, 0, c, N, mode, io[0]);
        else hipLaunchKernelGGL(k_staged, grid, block, lds, 0, c, N, mode, io[1]);
    };
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0)); CHECK(hipEventCreate(&t1));
    const int reps = 2000, rounds = 5;
    const char* names[2] = {"per-lane", "staged"};
    for (int mode : {1, 2, 3}) {
        std::vector<float> us[2];
        for (int v = 0; v < 2; ++v) {  // warm-up; mode 2 reads what a mode 1 launch left
            launch(v, 1);
            for (int k = 0; k < 20; ++k) launch(v, mode);
        }
        CHECK(hipDeviceSynchronize());
        for (int r = 0; r < rounds; ++r)
            for (int v = 0; v < 2; ++v) {
                CHECK(hipEventRecord(t0, 0));
                for (int k = 0; k < reps; ++k) launch(v, mode);
                CHECK(hipEventRecord(t1, 0));
                CHECK(hipEventSynchronize(t1));
                float ms = 0.0f;
                CHECK(hipEventElapsedTime(&ms, t0, t1));
                us[v].push_back(ms * 1000.0f / reps);
            }
        CHECK(hipGetLastError());
        for (int v = 0; v < 2; ++v) {
            std::sort(us[v].begin(), us[v].end());
            printf("N=%lld mode=%d %-8s median %.3f us/launch (min %.3f, max %.3f; %d launches x %d rounds)\n", (long long)N, mode, names[v],
                   us[v][rounds / 2], us[v].front(), us[v].back(), reps, rounds);
        }
    }
    std::vector<float> h[2];
    for (int v = 0; v < 2; ++v) {
        h[v].resize(N * 14);
        CHECK(hipMemcpy(h[v].data(), pd[v], N * 3 * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h[v].data() + N * 3, qd[v], N * 4 * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(h[v].data() + N * 7, jd[v], N * 7 * 4, hipMemcpyDeviceToHost));
    }
    const bool same = memcmp(h[0].data(), h[1].data(), h[0].size() * 4) == 0;
    printf("outputs of the two layouts %s\n", same ? "are bit-identical" : "DIFFER");
    return same ? 0 : 1;
}
