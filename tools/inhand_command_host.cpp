// CPU check of the in-hand command's arithmetic: runs inhand_command_env (isaaclab_amd/csrc/imx_inhand_command.h), the same code the
// gfx950 kernel k_inhand_command runs per lane, as plain host C++ over a flat binary file of inputs and writes a flat file of outputs.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/inhand_command_host.cpp -o inhand_command_host   (add -fsanitize=address,undefined while developing)
//   inhand_command_host IN OUT
//
// IN  = int32 header[8] {magic 0x31434849 "IHC1", N, steps, make_quat_unique, update_goal_on_success, 0, 0, 0}, fp32 cfg[4]
//       (imx_inhand_command_t.cfg), fp32 dt, fp32 pos_command_e (N,3), fp32 pos_command_w (N,3); then per step: int32 do_compute, fp32
//       object_root_pos_w (N,3), fp32 object_root_quat_w (N,4), int32 reset mask (N), fp32 uniforms (3,N,3).
// OUT = per step, the term's state after reset(mask) [+ compute(dt)]: fp32 command (N,7), time_left (N), orientation_error (N),
//       position_error (N), consecutive_success (N), then int64 command_counter (N).  The state starts as the constructor leaves it
//       (goal quaternion (1, 0, 0, 0), everything else zero) and persists from step to step.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../isaaclab_amd/csrc/imx_inhand_command.h"

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
    if (!read_exact(in, h, sizeof h) || h[0] != 0x31434849) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1];
    const int steps = h[2];
    if (N <= 0 || N > (1 << 20) || steps < 0) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    imx_inhand_command_t c{};
    c.make_quat_unique = h[3];
    c.update_goal_on_success = h[4];
    float dt;
    std::vector<float> pos_e(N * 3), pos_w(N * 3);
    if (!read_exact(in, c.cfg, sizeof c.cfg) || !read_exact(in, &dt, sizeof dt) || !read_exact(in, pos_e.data(), pos_e.size() * 4) ||
        !read_exact(in, pos_w.data(), pos_w.size() * 4)) {
        fprintf(stderr, "%s: the term's constant inputs are truncated\n", argv[1]);
        return 2;
    }
    std::vector<float> cmd(N * 7, 0.0f), tl(N, 0.0f), m_ori(N, 0.0f), m_pos(N, 0.0f), m_succ(N, 0.0f);
    std::vector<float> obj_pos(N * 3), obj_quat(N * 4), U(3 * N * 3);
    std::vector<int64_t> counter(N, 0);
    std::vector<int32_t> mask(N);
    std::vector<uint8_t> mask8(N);
    for (int64_t e = 0; e < N; ++e) {
        for (int k = 0; k < 3; ++k) cmd[e * 7 + k] = pos_e[e * 3 + k];
        cmd[e * 7 + 3] = 1.0f;
    }
    c.pos_command_w_d = pos_w.data();
    c.object_root_pos_w_d = obj_pos.data();
    c.object_root_quat_w_d = obj_quat.data();
    c.reset_mask_d = mask8.data();
    c.uniforms_d = U.data();
    c.command_d = cmd.data(); c.time_left_d = tl.data(); c.command_counter_d = counter.data();
    c.metric_orientation_error_d = m_ori.data(); c.metric_position_error_d = m_pos.data(); c.metric_consecutive_success_d = m_succ.data();
    if (const char* why = inhand_command_check(&c, 1)) {
        fprintf(stderr, "%s: %s\n", argv[1], why);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    for (int k = 0; k < steps; ++k) {
        int32_t do_compute;
        if (!read_exact(in, &do_compute, 4) || !read_exact(in, obj_pos.data(), obj_pos.size() * 4) ||
            !read_exact(in, obj_quat.data(), obj_quat.size() * 4) || !read_exact(in, mask.data(), mask.size() * 4) ||
            !read_exact(in, U.data(), U.size() * 4)) {
            fprintf(stderr, "%s: step %d is truncated\n", argv[1], k);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e) {
            float m0[3];
            inhand_command_env(N, e, c, dt, do_compute != 0, mask[e] != 0, 0, m0);
        }
        fwrite(cmd.data(), 4, cmd.size(), out); fwrite(tl.data(), 4, tl.size(), out); fwrite(m_ori.data(), 4, m_ori.size(), out);
        fwrite(m_pos.data(), 4, m_pos.size(), out); fwrite(m_succ.data(), 4, m_succ.size(), out);
        fwrite(counter.data(), 8, counter.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
