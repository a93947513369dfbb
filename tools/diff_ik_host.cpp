// CPU check of the differential-IK kernel's arithmetic: runs diff_ik_env (isaaclab_amd/csrc/imx_diff_ik.h), the same code the gfx950
// kernel runs per lane, as plain host C++ over a flat binary file of inputs and writes a flat file of outputs.
//
//   c++ -O2 -std=c++17 -ffp-contract=off tools/diff_ik_host.cpp -o diff_ik_host        (add -fsanitize=address,undefined while developing)
//   diff_ik_host IN OUT
//
// IN  = int32 header[8] {magic 0x314B4944 "DIK1", N, PA, num_bodies, NB, ND, J, ncalls}, the raw bytes of one imx_diff_ik_t, then per
//       call: int32 mode, and fp32 processed_action (N,PA), root_pos_w (N,3), root_quat_w (N,4), body_pos_w (N,num_bodies,3),
//       body_quat_w (N,num_bodies,4), jacobians (N,NB,6,ND), joint_pos (N,J).
// OUT = per call, the three outputs as they stand after it: ee_pos_des (N,3), ee_quat_des (N,4), joint_pos_des (N,num_joints).  They
//       start as zeros and persist from call to call, as the env's tensors do.
// The same argument checks as imx_diff_ik run before every call; a refused call ends the program with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../isaaclab_amd/csrc/imx_diff_ik.h"

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
    imx_diff_ik_t cfg;
    if (!read_exact(in, h, sizeof h) || h[0] != 0x314B4944 || !read_exact(in, &cfg, sizeof cfg)) {
        fprintf(stderr, "%s: bad header\n", argv[1]);
        return 2;
    }
    const int64_t N = h[1], PA = h[2], B = h[3], NB = h[4], ND = h[5], J = h[6];
    const int ncalls = h[7];
    const int64_t lim = 1 << 20;
    if (N <= 0 || N > lim || PA <= 0 || PA > lim || B <= 0 || B > lim || NB <= 0 || NB > lim || ND <= 0 || ND > lim || J <= 0 || J > lim ||
        ncalls < 0 || N * NB * 6 * ND > (1ll << 28) || cfg.num_joints < 1 || cfg.num_joints > IMX_IK_MAX_JOINTS) {
        fprintf(stderr, "%s: sizes out of range\n", argv[1]);
        return 2;
    }
    const int n = cfg.num_joints;
    std::vector<float> act(N * PA), rp(N * 3), rq(N * 4), bp(N * B * 3), bq(N * B * 4), jac(N * NB * 6 * ND), jp(N * J);
    std::vector<float> pos_des(N * 3, 0.0f), quat_des(N * 4, 0.0f), q_des(N * n, 0.0f);
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    for (int k = 0; k < ncalls; ++k) {
        int32_t mode;
        if (!read_exact(in, &mode, sizeof mode) || !read_exact(in, act.data(), act.size() * 4) || !read_exact(in, rp.data(), rp.size() * 4) ||
            !read_exact(in, rq.data(), rq.size() * 4) || !read_exact(in, bp.data(), bp.size() * 4) || !read_exact(in, bq.data(), bq.size() * 4) ||
            !read_exact(in, jac.data(), jac.size() * 4) || !read_exact(in, jp.data(), jp.size() * 4)) {
            fprintf(stderr, "%s: call %d is truncated\n", argv[1], k);
            return 2;
        }
        const DiffIkIO io{act.data(), PA, rp.data(), rq.data(), bp.data(), bq.data(), B, jac.data(), NB, ND, jp.data(), J,
                          pos_des.data(), quat_des.data(), q_des.data(), n};
        if (const char* why = imx_diff_ik_check(&cfg, N, mode, io)) {
            fprintf(stderr, "call %d refused: %s\n", k, why);
            return 2;
        }
        for (int64_t e = 0; e < N; ++e)
            diff_ik_env(cfg, e, mode, io, (mode & 2) ? jac.data() + (e * NB + cfg.jacobi_body_idx) * 6 * ND : nullptr);
        fwrite(pos_des.data(), 4, pos_des.size(), out);
        fwrite(quat_des.data(), 4, quat_des.size(), out);
        fwrite(q_des.data(), 4, q_des.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
