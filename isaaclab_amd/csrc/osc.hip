// OperationalSpaceControllerAction (envs/mdp/actions/task_space_actions.py:232-700): the stand-alone entry point imx_osc.
// Lane = env, no atomics, one wave per block (a few thousand envs are latency-bound: 64-lane blocks spread them over the CUs, and a
// block of one wave lets an instantiation use the whole register file: DESIGN.md "Operational-space controller" has the figures).
// The arithmetic of one env is osc_env (imx_osc.h); the decoupling and the null-space projection are compile-time, so that the
// cfg without a mass matrix carries no factor and only the redundant full-decoupling cfg carries the second solve.
#include "imx_osc.h"
#include "imx_internal.h"

template <int DEC, bool NULLSP>
__global__ void __launch_bounds__(IMX_WAVE)
k_osc(imx_osc_t c, int64_t N, int mode, OscIO io) {
    const int64_t e = (int64_t)blockIdx.x * IMX_WAVE + threadIdx.x;
    if (e >= N) return;
    osc_env<DEC, NULLSP>(c, e, mode, io);
}

extern "C" int imx_osc(const imx_osc_t* cfg, int64_t N, int mode, const float* processed_action_d, int64_t PA,
                       const float* root_pos_w_d, const float* root_quat_w_d, const float* root_lin_vel_w_d, const float* root_ang_vel_w_d,
                       const float* body_pos_w_d, const float* body_quat_w_d, const float* body_lin_vel_w_d, const float* body_ang_vel_w_d,
                       int64_t num_bodies, const float* jacobians_d, int64_t NB, int64_t ND, const float* mass_matrices_d, const float* gravity_d,
                       int64_t NM, const float* joint_pos_d, const float* joint_vel_d, int64_t J, const float* nullspace_target_d,
                       float* command_state_d, int64_t ld_cmd, float* joint_efforts_d, int64_t ld_eff, imx_stream_t stream) {
    const OscIO io{processed_action_d, PA, root_pos_w_d, root_quat_w_d, root_lin_vel_w_d, root_ang_vel_w_d, body_pos_w_d, body_quat_w_d,
                   body_lin_vel_w_d, body_ang_vel_w_d, num_bodies, jacobians_d, NB, ND, mass_matrices_d, gravity_d, NM, joint_pos_d, joint_vel_d, J,
                   nullspace_target_d, command_state_d, ld_cmd, joint_efforts_d, ld_eff};
    const char* why = imx_osc_check(cfg, N, mode, io);
    IMX_REQUIRE(!why, "imx_osc: %s", why);
    const dim3 grid((unsigned)((N + IMX_WAVE - 1) / IMX_WAVE)), block(IMX_WAVE);
    hipStream_t s = (hipStream_t)stream;
    if (cfg->decoupling == IMX_OSC_DECOUPLING_FULL && cfg->nullspace_position)
        hipLaunchKernelGGL((k_osc<IMX_OSC_DECOUPLING_FULL, true>), grid, block, 0, s, *cfg, N, mode, io);
    else if (cfg->decoupling == IMX_OSC_DECOUPLING_FULL)
        hipLaunchKernelGGL((k_osc<IMX_OSC_DECOUPLING_FULL, false>), grid, block, 0, s, *cfg, N, mode, io);
    else if (cfg->decoupling == IMX_OSC_DECOUPLING_PARTIAL)
        hipLaunchKernelGGL((k_osc<IMX_OSC_DECOUPLING_PARTIAL, false>), grid, block, 0, s, *cfg, N, mode, io);
    else
        hipLaunchKernelGGL((k_osc<IMX_OSC_DECOUPLING_NONE, false>), grid, block, 0, s, *cfg, N, mode, io);
    IMX_HIP(hipGetLastError());
    return 0;
}
