// DifferentialInverseKinematicsAction (envs/mdp/actions/task_space_actions.py:30-229): the stand-alone entry point imx_diff_ik.
// Lane = env, no atomics, one wave per block (a few thousand envs are latency-bound: 64-lane blocks spread them over the CUs).
// The arithmetic of one env is diff_ik_env (imx_diff_ik.h).
#include "imx_diff_ik.h"
#include "imx_internal.h"

// Each lane reads its own 6 x ND Jacobian block straight from global memory: 6 * num_joints independent loads per lane, issued back
// to back (DESIGN.md "Differential IK" has the measurement against a copy staged through LDS).
__global__ void __launch_bounds__(IMX_WAVE)
k_diff_ik(imx_diff_ik_t c, int64_t N, int mode, DiffIkIO io) {
    const int64_t e = (int64_t)blockIdx.x * IMX_WAVE + threadIdx.x;
    if (e >= N) return;
    const float* jrow = (mode & 2) ? io.jacobians + (e * io.NB + c.jacobi_body_idx) * 6 * io.ND : nullptr;
    diff_ik_env(c, e, mode, io, jrow);
}

extern "C" int imx_diff_ik(const imx_diff_ik_t* cfg, int64_t N, int mode, const float* processed_action_d, int64_t PA,
                           const float* root_pos_w_d, const float* root_quat_w_d, const float* body_pos_w_d, const float* body_quat_w_d,
                           int64_t num_bodies, const float* jacobians_d, int64_t NB, int64_t ND, const float* joint_pos_d, int64_t J,
                           float* ee_pos_des_d, float* ee_quat_des_d, float* joint_pos_des_d, int64_t ld_des, imx_stream_t stream) {
    const DiffIkIO io{processed_action_d, PA, root_pos_w_d, root_quat_w_d, body_pos_w_d, body_quat_w_d, num_bodies, jacobians_d, NB, ND,
                      joint_pos_d, J, ee_pos_des_d, ee_quat_des_d, joint_pos_des_d, ld_des};
    const char* why = imx_diff_ik_check(cfg, N, mode, io);
    IMX_REQUIRE(!why, "imx_diff_ik: %s", why);
    hipLaunchKernelGGL(k_diff_ik, dim3((unsigned)((N + IMX_WAVE - 1) / IMX_WAVE)), dim3(IMX_WAVE), 0, (hipStream_t)stream, *cfg, N, mode, io);
    IMX_HIP(hipGetLastError());
    return 0;
}
