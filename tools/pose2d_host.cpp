// CPU check of the pose-2d command's arithmetic: runs pose2d_command_env (isaaclab_amd/csrc/imx_pose2d.h), the same code the gfx950
// kernels k_pose2d_command and k_reset_orchestrate_pose2d run per lane, as plain host C++ over a flat binary file of inputs and writes a
// flat file of outputs.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/pose2d_host.cpp -o pose2d_host   (add -fsanitize=address,undefined while developing)
//   pose2d_host IN OUT
//
// IN  = int32 header[8] {magic 0x31443250 "P2D1", N, steps, kind, simple_heading, L, T, P}, fp32 cfg[8] (imx_pose2d_command_t.cfg),
//       fp32 dt, fp32 env_origins (N,3), fp32 default_root_z (N), with kind 1: fp32 valid_targets (L,T,P,3), int64 terrain_levels (N),
//       int64 terrain_types (N); then per step: fp32 root_pos_w (N,3), fp32 root_quat_w (N,4), int32 reset mask (N), fp32 uniforms
//       (2,N,4), with kind 1: int64 patch_ids (2,N).
// OUT = per step, the term's state after reset(mask) + compute(dt): fp32 command (N,4), pos_command_w (N,3), heading_command_w (N),
//       time_left (N), error_pos_2d (N), error_heading (N), then int64 command_counter (N).  The state starts as zeros and persists from
//       step to step.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../isaaclab_amd/csrc/imx_pose2d.h"

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
    int32_t h[8];
    if (!read_exact(in, h, sizeof h) || h[0] != 0x31443250) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1];
    const int steps = h[2], kind = h[3];
    const int64_t L = h[5], T = h[6], P = h[7];
    if (N <= 0 || N > (1 << 20) || steps < 0 || (kind != 0 && kind != 1) ||
        (kind == 1 && (L <= 0 || T <= 0 || P <= 0 || L > 1024 || T > 1024 || P > 1024))) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    imx_pose2d_command_t c{};
    c.kind = kind;
    c.simple_heading = h[4];
    float dt;
    std::vector<float> origins(N * 3), z(N), targets(kind == 1 ? L * T * P * 3 : 0);
    std::vector<int64_t> levels(kind == 1 ? N : 0), types(kind == 1 ? N : 0), patch(kind == 1 ? 2 * N : 0);
    if (!read_exact(in, c.cfg, sizeof c.cfg) || !read_exact(in, &dt, sizeof dt) || !read_exact(in, origins.data(), origins.size() * 4) ||
        !read_exact(in, z.data(), z.size() * 4) || !read_exact(in, targets.data(), targets.size() * 4) ||
        !read_exact(in, levels.data(), levels.size() * 8) || !read_exact(in, types.data(), types.size() * 8)) {
        fprintf(stderr, "%s: the term's constant inputs are truncated\n", argv[1]);
        return 2;
    }
    for (int64_t e = 0; e < (kind == 1 ? N : 0); ++e)
        if (levels[e] < 0 || levels[e] >= L || types[e] < 0 || types[e] >= T) {
            fprintf(stderr, "%s: env %lld has a terrain level or type outside the table\n", argv[1], (long long)e);
            return 2;
        }
    std::vector<float> cmd(N * 4, 0.0f), pw(N * 3, 0.0f), hw(N, 0.0f), tl(N, 0.0f), mpos(N, 0.0f), mhead(N, 0.0f);
    std::vector<float> root_pos(N * 3), root_quat(N * 4), U(2 * N * 4);
    std::vector<int64_t> counter(N, 0);
    std::vector<int32_t> mask(N);
    c.env_origins_d = origins.data();
    c.default_root_z_d = z.data();
    if (kind == 1) {
        c.valid_targets_d = targets.data();
        c.terrain_levels_d = levels.data();
        c.terrain_types_d = types.data();
        c.num_levels = (int32_t)L; c.num_types = (int32_t)T; c.num_patches = (int32_t)P;
        c.patch_ids_d = patch.data();
    }
    c.uniforms_d = U.data();
    c.command_d = cmd.data(); c.pos_command_w_d = pw.data(); c.heading_command_w_d = hw.data(); c.time_left_d = tl.data();
    c.command_counter_d = counter.data(); c.metric_error_pos_2d_d = mpos.data(); c.metric_error_heading_d = mhead.data();
    if (const char* why = pose2d_command_check(&c)) {
        fprintf(stderr, "%s: %s\n", argv[1], why);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    for (int k = 0; k < steps; ++k) {
        if (!read_exact(in, root_pos.data(), root_pos.size() * 4) || !read_exact(in, root_quat.data(), root_quat.size() * 4) ||
            !read_exact(in, mask.data(), mask.size() * 4) || !read_exact(in, U.data(), U.size() * 4) || !read_exact(in, patch.data(), patch.size() * 8)) {
            fprintf(stderr, "%s: step %d is truncated\n", argv[1], k);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e) {
            float m0, m1;
            pose2d_command_env(N, e, c, dt, 1, root_pos.data(), root_quat.data(), mask[e] != 0, 0, 0, m0, m1);
        }
        fwrite(cmd.data(), 4, cmd.size(), out); fwrite(pw.data(), 4, pw.size(), out); fwrite(hw.data(), 4, hw.size(), out);
        fwrite(tl.data(), 4, tl.size(), out); fwrite(mpos.data(), 4, mpos.size(), out); fwrite(mhead.data(), 4, mhead.size(), out);
        fwrite(counter.data(), 8, counter.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
