// The per-env arithmetic of the two root-state reset events (envs/mdp/events.py:823-868 reset_root_state_uniform, :1096-1118
// reset_scene_to_default).  Shared by the orchestration kernel (orchestrate.hip), which runs it for the robot and for the scene's rigid
// object, and by the host program tools/manip_orch_host.cpp: this file compiles as gfx950 device code and as plain host C++.
#pragma once
#include <math.h>

#include "imx_quat.h"

// reset_root_state_uniform (:843-865) for one env.  d: the asset's default root state (13); o: scene.env_origins of the env; rs: the six
// pose samples (x, y, z, roll, pitch, yaw), already scaled to their ranges.  pose (7) = position default + origin + sample, orientation
// quat_mul(default, quat_from_euler_xyz(roll, pitch, yaw)) (utils/math.py:266-276, 486-497; the same association).
IMX_HD void root_pose_uniform_env(const float* d, float ox, float oy, float oz, const float* rs, float* pose) {
    pose[0] = d[0] + ox + rs[0];  // positions = default + env origin + sample (:852)
    pose[1] = d[1] + oy + rs[1];
    pose[2] = d[2] + oz + rs[2];
    const float cy = cosf(rs[5] * 0.5f), sy = sinf(rs[5] * 0.5f), cr = cosf(rs[3] * 0.5f), sr = sinf(rs[3] * 0.5f);
    const float cp = cosf(rs[4] * 0.5f), sp = sinf(rs[4] * 0.5f);
    const float w2 = cy * cr * cp + sy * sr * sp, x2 = cy * sr * cp - sy * cr * sp, y2 = cy * cr * sp + sy * sr * cp,
                z2 = sy * cr * cp - cy * sr * sp;
    const float w1 = d[3], x1 = d[4], y1 = d[5], z1 = d[6];
    const float ww = (z1 + x1) * (x2 + y2), yy = (w1 - y1) * (w2 + z2), zz = (w1 + y1) * (w2 - z2);
    const float xx = ww + yy + zz;
    const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
    pose[3] = qq - ww + (z1 - y1) * (y2 - z2);
    pose[4] = qq - xx + (x1 + w1) * (x2 + w2);
    pose[5] = qq - yy + (w1 - x1) * (y2 + z2);
    pose[6] = qq - zz + (z1 + y1) * (w2 - x2);
}

// reset_joints_by_offset / reset_joints_by_scale (:987-1049) for one joint of one env of the scene's second articulation: up, uv the two
// samples in [0,1) (columns j and J2 + j), r = {position lo, hi, velocity lo, hi}.  default (+ | *) sample, then clamp_(lo, hi) to the
// soft position limits and to +- the soft velocity limit -- the arithmetic of the robot's path in orchestrate.hip, term by term
IMX_HD void joint_reset_env(bool by_offset, float dp, float dv, float up, float uv, const float* r, float plo, float phi, float vlim, float* p,
                            float* v) {
    const float sp = up * (r[1] - r[0]) + r[0];
    const float sv = uv * (r[3] - r[2]) + r[2];
    const float pp = by_offset ? dp + sp : dp * sp;
    const float vv = by_offset ? dv + sv : dv * sv;
    *p = fminf(fmaxf(pp, plo), phi);
    *v = fminf(fmaxf(vv, -vlim), vlim);
}

// reset_root_state_uniform's velocity (:857-865) for one env: vel (6) = default[7:] + sample, u6 the six samples in [0,1) (columns
// 6..11), r the six velocity ranges lo, hi
IMX_HD void root_vel_uniform_env(const float* d, const float* u6, const float* r, float* vel) {
    for (int k = 0; k < 6; ++k) vel[k] = d[7 + k] + (u6[k] * (r[2 * k + 1] - r[2 * k]) + r[2 * k]);
}

// reset_scene_to_default (:1099-1113) for one asset of one env: pose (7) = default[:7] with the env origin added to the position,
// vel (6) = default[7:]
IMX_HD void root_state_default_env(const float* d, float ox, float oy, float oz, float* pose, float* vel) {
    pose[0] = d[0] + ox;
    pose[1] = d[1] + oy;
    pose[2] = d[2] + oz;
    for (int k = 3; k < 7; ++k) pose[k] = d[k];
    for (int k = 0; k < 6; ++k) vel[k] = d[7 + k];
}
