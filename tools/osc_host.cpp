// CPU check of the operational-space kernel's arithmetic: runs osc_env (isaaclab_amd/csrc/imx_osc.h), the same code the gfx950 kernel
// runs per lane, as plain host C++ over a flat binary file of inputs and writes a flat file of outputs.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/osc_host.cpp -o osc_host        (add -fsanitize=address,undefined while developing)
//   osc_host IN OUT
//
// IN  = int32 header[12] {magic 0x3143534F "OSC1", N, PA, num_bodies, NB, ND, NM, J, ncalls, 0, 0, 0}, the raw bytes of one imx_osc_t,
//       fp32 nullspace_target (N, num_joints), then per call: int32 mode, and fp32 processed_action (N,PA), root_pos_w (N,3), root_quat_w
//       (N,4), root_lin_vel_w (N,3), root_ang_vel_w (N,3), body_pos_w (N,num_bodies,3), body_quat_w (N,num_bodies,4), body_lin_vel_w,
//       body_ang_vel_w (N,num_bodies,3), jacobians (N,NB,6,ND), mass_matrices (N,NM,NM), gravity (N,NM), joint_pos (N,J), joint_vel (N,J).
// OUT = per call, the two outputs as they stand after it: command_state (N,25), joint_efforts (N,num_joints).  They start as zeros and
//       persist from call to call, as the env's tensors do.
// The same argument checks as imx_osc run before every call; a refused call ends the program with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../isaaclab_amd/csrc/imx_osc.h"

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
    int32_t h[12];
    imx_osc_t cfg;
    if (!read_exact(in, h, sizeof h) || h[0] != 0x3143534F || !read_exact(in, &cfg, sizeof cfg)) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1], PA = h[2], B = h[3], NB = h[4], ND = h[5], NM = h[6], J = h[7];
    const int ncalls = h[8];
    const int64_t lim = 1 << 20;
    if (N <= 0 || N > lim || PA <= 0 || PA > lim || B <= 0 || B > lim || NB <= 0 || NB > lim || ND <= 0 || ND > lim || NM <= 0 || NM > 1024 ||
        J <= 0 || J > lim || ncalls < 0 || N * NB * 6 * ND > (1ll << 28) || N * NM * NM > (1ll << 28) || cfg.num_joints < 1 ||
        cfg.num_joints > IMX_IK_MAX_JOINTS) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    const int n = cfg.num_joints;
    std::vector<float> target(N * n), act(N * PA), rp(N * 3), rq(N * 4), rlv(N * 3), rav(N * 3), bp(N * B * 3), bq(N * B * 4), blv(N * B * 3),
        bav(N * B * 3), jac(N * NB * 6 * ND), mass(N * NM * NM), grav(N * NM), jp(N * J), jv(N * J);
    std::vector<float> cmd(N * IMX_OSC_CMD_WIDTH, 0.0f), eff(N * n, 0.0f);
    if (!read_exact(in, target.data(), target.size() * 4)) {
        fprintf(stderr, "%s: no null-space target\n", argv[1]);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    std::vector<float>* per_call[] = {&act, &rp, &rq, &rlv, &rav, &bp, &bq, &blv, &bav, &jac, &mass, &grav, &jp, &jv};
    for (int k = 0; k < ncalls; ++k) {
        int32_t mode;
        bool ok = read_exact(in, &mode, sizeof mode);
        for (auto* v : per_call) ok = ok && read_exact(in, v->data(), v->size() * 4);
        if (!ok) {
            fprintf(stderr, "%s: call %d is truncated\n", argv[1], k);
            return 2;
        }
        const OscIO io{act.data(), PA, rp.data(), rq.data(), rlv.data(), rav.data(), bp.data(), bq.data(), blv.data(), bav.data(), B,
                       jac.data(), NB, ND, mass.data(), grav.data(), NM, jp.data(), jv.data(), J, target.data(),
                       cmd.data(), IMX_OSC_CMD_WIDTH, eff.data(), n};
        if (const char* why = imx_osc_check(&cfg, N, mode, io)) {
            fprintf(stderr, "call %d refused: %s\n", k, why);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e) osc_env_dispatch(cfg, e, mode, io);
        fwrite(cmd.data(), 4, cmd.size(), out);
        fwrite(eff.data(), 4, eff.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
