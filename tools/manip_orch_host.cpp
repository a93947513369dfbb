// CPU check of the root-state reset events' arithmetic: runs root_pose_uniform_env / root_state_default_env
// (isaaclab_amd/csrc/imx_manip_events.h), the same code the gfx950 orchestration kernel runs per lane for the robot and for the scene's
// rigid object, as plain host C++ over a flat binary file of inputs and writes a flat file of outputs.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/manip_orch_host.cpp -o manip_orch_host   (add -fsanitize=address,undefined while developing)
//   manip_orch_host IN OUT
//
// IN  = int32 header[4] {magic 0x31504E4D "MNP1", N, ncalls, 0}, fp32 default_root_state (N,13), fp32 env_origins (N,3), then per call:
//       int32 op (0 = reset_scene_to_default's write for this asset, 1 = reset_root_state_uniform), fp32 ranges[24] (pose lo/hi x 6,
//       velocity lo/hi x 6), int32 mask (N) (the envs the event runs on), fp32 uniforms (N,12) in [0,1).
// OUT = per call, the asset's two "to simulator" buffers as they stand after it: pose (N,7), velocity (N,6).  They start as zeros and
//       persist from call to call, as the env's tensors do; rows outside the mask are not touched.
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
    if (!read_exact(in, h, sizeof h) || h[0] != 0x31504E4D) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1];
    const int ncalls = h[2];
    if (N <= 0 || N > (1 << 20) || ncalls < 0) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    std::vector<float> def(N * 13), org(N * 3), u(N * 12), pose(N * 7, 0.0f), vel(N * 6, 0.0f);
    std::vector<int32_t> mask(N);
    if (!read_exact(in, def.data(), def.size() * 4) || !read_exact(in, org.data(), org.size() * 4)) {
        fprintf(stderr, "%s: no default root state / env origins\n", argv[1]);
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
        if (!read_exact(in, &op, sizeof op) || (op != 0 && op != 1) || !read_exact(in, r, sizeof r) || !read_exact(in, mask.data(), mask.size() * 4) ||
            !read_exact(in, u.data(), u.size() * 4)) {
            fprintf(stderr, "%s: call %d is truncated or names an unknown op\n", argv[1], k);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e) {
            if (!mask[e]) continue;
            const float *d = &def[e * 13], *o = &org[e * 3];
            if (op == 0) {
                root_state_default_env(d, o[0], o[1], o[2], &pose[e * 7], &vel[e * 6]);
                continue;
            }
            float rs[6];
            for (int c = 0; c < 6; ++c) rs[c] = u[e * 12 + c] * (r[2 * c + 1] - r[2 * c]) + r[2 * c];
            root_pose_uniform_env(d, o[0], o[1], o[2], rs, &pose[e * 7]);
            for (int c = 0; c < 6; ++c) vel[e * 6 + c] = d[7 + c] + (u[e * 12 + 6 + c] * (r[12 + 2 * c + 1] - r[12 + 2 * c]) + r[12 + 2 * c]);
        }
        fwrite(pose.data(), 4, pose.size(), out);
        fwrite(vel.data(), 4, vel.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
