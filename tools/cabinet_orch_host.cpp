// CPU check of the reset events' arithmetic on one articulation of the scene (the robot or the second one, the Open-Drawer task's
// cabinet): runs root_state_default_env / root_pose_uniform_env / root_vel_uniform_env / joint_reset_env
// (isaaclab_amd/csrc/imx_manip_events.h), the same code the gfx950 orchestration kernel (k_reset_orchestrate_scene) runs for the second
// articulation, as plain host C++ over a flat binary file of inputs and writes a flat file of outputs.  Sibling of manip_orch_host.cpp.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/cabinet_orch_host.cpp -o cabinet_orch_host   (add -fsanitize=address,undefined while developing)
//   cabinet_orch_host IN OUT
//
// IN  = int32 header[4] {magic 0x31424143 "CAB1", N, J, ncalls}, fp32 default_root_state (N,13), env_origins (N,3), default_joint_pos (N,J),
//       default_joint_vel (N,J), soft_joint_pos_limits (N,J,2), soft_joint_vel_limits (N,J), then per call: int32 op (0 = reset_scene_to_default's
//       writes for this asset, 1 = reset_root_state_uniform, 2 = reset_joints_by_offset, 3 = reset_joints_by_scale), fp32 ranges[24] (op 1:
//       pose lo/hi x 6, velocity lo/hi x 6; op 2, 3: position lo, hi, velocity lo, hi), int32 mask (N) (the envs the event runs on),
//       fp32 uniforms (N,W) in [0,1), W = max(12, 2 J) (op 1 reads 12 columns, op 2, 3 read 2 J).
// OUT = per call, the asset's four "to simulator" buffers as they stand after it: pose (N,7), velocity (N,6), joint_pos (N,J), joint_vel
//       (N,J).  They start as zeros and persist from call to call, as the env's tensors do; rows outside the mask are not touched.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../isaaclab_amd/csrc/imx_manip_events.h"

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t h[4];
    if (!read_exact(in, h, sizeof h) || h[0] != 0x31424143) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1], J = h[2];
    const int ncalls = h[3];
    if (N <= 0 || N > (1 << 20) || J <= 0 || J > 4096 || ncalls < 0) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    const int64_t W = 2 * J > 12 ? 2 * J : 12;
    std::vector<float> def(N * 13), org(N * 3), djp(N * J), djv(N * J), lim(N * J * 2), vlim(N * J), u(N * W);
    std::vector<float> pose(N * 7, 0.0f), vel(N * 6, 0.0f), jp(N * J, 0.0f), jv(N * J, 0.0f);
    std::vector<int32_t> mask(N);
    if (!read_exact(in, def.data(), def.size() * 4) || !read_exact(in, org.data(), org.size() * 4) || !read_exact(in, djp.data(), djp.size() * 4) ||
        !read_exact(in, djv.data(), djv.size() * 4) || !read_exact(in, lim.data(), lim.size() * 4) || !read_exact(in, vlim.data(), vlim.size() * 4)) {
        fprintf(stderr, "%s: the defaults / limits are truncated\n", argv[1]);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    for (int k = 0; k < ncalls; ++k) {
        int32_t op;
        float r[24];
        if (!read_exact(in, &op, sizeof op) || op < 0 || op > 3 || !read_exact(in, r, sizeof r) || !read_exact(in, mask.data(), mask.size() * 4) ||
            !read_exact(in, u.data(), u.size() * 4)) {
            fprintf(stderr, "%s: call %d is truncated or names an unknown op\n", argv[1], k);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e) {
            if (!mask[e]) continue;
            const float *d = &def[e * 13], *o = &org[e * 3], *ue = &u[e * W];
            if (op == 0) {
                root_state_default_env(d, o[0], o[1], o[2], &pose[e * 7], &vel[e * 6]);
                for (int64_t j = 0; j < J; ++j) {
                    jp[e * J + j] = djp[e * J + j];
                    jv[e * J + j] = djv[e * J + j];
                }
            } else if (op == 1) {
                float rs[6];
                for (int c = 0; c < 6; ++c) rs[c] = ue[c] * (r[2 * c + 1] - r[2 * c]) + r[2 * c];
                root_pose_uniform_env(d, o[0], o[1], o[2], rs, &pose[e * 7]);
                root_vel_uniform_env(d, ue + 6, r + 12, &vel[e * 6]);
            } else {
                for (int64_t j = 0; j < J; ++j) {
                    const int64_t q = e * J + j;
                    joint_reset_env(op == 2, djp[q], djv[q], ue[j], ue[J + j], r, lim[2 * q], lim[2 * q + 1], vlim[q], &jp[q], &jv[q]);
                }
            }
        }
        fwrite(pose.data(), 4, pose.size(), out);
        fwrite(vel.data(), 4, vel.size(), out);
        fwrite(jp.data(), 4, jp.size(), out);
        fwrite(jv.data(), 4, jv.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
