// k_inhand_command: the in-hand re-orientation command term (InHandReOrientationCommand, isaaclab_tasks .../manipulation/inhand/mdp/
// commands/orientation_command.py) under CommandTerm.reset / compute, one lane per env, ONE launch for a reset on a mask and / or a
// compute(dt).  The per-env arithmetic is inhand_command_env (imx_inhand_command.h, shared with tools/inhand_command_host.cpp).
#include "imx_internal.h"
#include "imx_inhand_command.h"

static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lane = env; no LDS, no atomics.  With log_part the 64-lane wave also leaves the sums of the reset envs' metrics as they stood (a
// fixed-shape shuffle tree: deterministic) and their count: the means CommandTerm.reset logs are sums over these rows
__global__ void __launch_bounds__(256)
k_inhand_command(int64_t N, imx_inhand_command_t c, float dt, int do_compute) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e < N;
    const bool reset = live && c.reset_mask_d && c.reset_mask_d[e];
    float m0[3] = {0.0f, 0.0f, 0.0f};
    if (live) inhand_command_env(N, e, c, dt, do_compute, reset, c.step_counter_d ? (uint32_t)c.step_counter_d[0] : 0u, m0);
    if (!c.log_part_d) return;
    const int64_t w = e >> 6;  // (whole waves run: the grid is padded to 256 lanes, dead lanes add zeros)
    if (w * 64 >= N) return;
    const float s0 = wave_sum(reset ? m0[0] : 0.0f), s1 = wave_sum(reset ? m0[1] : 0.0f), s2 = wave_sum(reset ? m0[2] : 0.0f);
    const float n = wave_sum(reset ? 1.0f : 0.0f);
    if ((threadIdx.x & 63) == 0) {
        float* o = c.log_part_d + w * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = n;
    }
}

extern "C" int imx_inhand_command(const imx_inhand_command_t* term, int64_t N, float dt, int flags, imx_stream_t stream) {
    IMX_REQUIRE(N > 0 && N < (1ll << 31), "imx_inhand_command: N out of range");
    IMX_REQUIRE((flags & ~1) == 0, "imx_inhand_command: unknown flags %d (bit 0 = compute)", flags);
    if (const char* why = inhand_command_check(term, flags & 1)) IMX_FAIL("imx_inhand_command: %s", why);
    IMX_REQUIRE(dt >= 0.0f, "imx_inhand_command: negative dt");
    hipLaunchKernelGGL(k_inhand_command, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, *term, dt, flags & 1);
    IMX_HIP(hipGetLastError());
    return 0;
}
