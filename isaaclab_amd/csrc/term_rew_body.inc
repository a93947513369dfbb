// The body of k_term_rew (step.hip), included once per kernel: in k_term_rew<CLASSIC, REACH> as it always was, and with IMX_TR_LIFT
// defined in k_term_rew_lift, IMX_TR_NAV in k_term_rew_nav, IMX_TR_INHAND in k_term_rew_inhand, IMX_TR_CABINET in k_term_rew_cabinet.  A textual include, not a device function: the kernels of the existing tasks then compile to the very
// instruction streams they had (a shared force-inlined body moved their register allocation and cost them 0.4 us per launch).
    extern __shared__ int32_t smem[];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    const int64_t grp = blockIdx.x;
    const int64_t e = grp * G + lane;
    const bool live = lane < G && e < N;
    const int64_t ec = live ? e : min(grp * G, N - 1);  // dead lanes compute on a valid env of the group (no extra cache lines), never store
    const int J = P.J, Bn = P.B, H = P.H, A = P.A;
    const int nterm = P.nterm, nrew = P.nrew;
    const int32_t* __restrict__ W = P.w;  // term tables: wave-uniform addresses -> scalar loads (L2-resident, a few KB)
    // The step counter (keys the in-kernel random streams, stamps the sensor rows) is advanced here without a read-modify-write race:
    // this kernel reads the shadow counters[3] the last observation launch left and publishes counters[2] = shadow + 1; the observation
    // kernel reads counters[2] and writes the shadow.
    const uint32_t step = (uint32_t)Bf.counters[3] + 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) Bf.counters[2] = (int32_t)step;
    IMX_STAMP(0);
    // LDS: [termination values: nterm x 64 u32 (bit 0 value, bit 1 time-out term)][f: nrew x 64][es: nrew x 64][val: nrew x 64];
    // every slot is written by exactly one wave before the barrier that publishes it: no zero fill, no atomics
    uint32_t* s_tv = reinterpret_cast<uint32_t*>(smem);
    float* s_f = reinterpret_cast<float*>(s_tv + (nterm > 0 ? nterm : 1) * 64);
    float* s_es = s_f + nrew * 64;
    float* s_val = s_es + nrew * 64;
#ifdef IMX_TR_INHAND
    // dtheta = quat_error_magnitude(object_root_quat_w, cmd[3:7]) of the env, once for all the terms that read it: the last wave (it has
    // the fewest items) leaves it in 64 more floats of LDS before the barrier that ends phase 1; the rewards read it in phase 2
    float* s_dth = s_val + nrew * 64;
    if (need_dtheta && wv == NW - 1) {
        const float* __restrict__ gq = S.command + ec * P.CMD + 3;
        s_dth[lane] = quat_error_magnitude(reinterpret_cast<const float4*>(X.object_root_quat_w)[ec], make_float4(gq[0], gq[1], gq[2], gq[3]));
    }
#endif
#ifdef IMX_TR_CABINET
    // the env's FrameTransformer frames, once for the seven cabinet rewards: the last wave leaves 20 floats per env in LDS before the
    // barrier that ends phase 1 -- rows 0-2 the tool centre point's position, 3-6 its quaternion, 7-9 the handle's position, 10-13 its
    // quaternion, 14-16 / 17-19 the left / right fingertip's position (fingers: a reward of the plan reads them); phase 2 reads them
    float* s_fr = s_val + nrew * 64;
    if (wv == NW - 1) {
        const int B2 = W[ft_off + 1], n_ee = W[ft_off + 2];
        const ImxFramePose tcp = cabinet_frame_pose(P, S, X, ft_ee_target(ft_off, 0), B2, ec);
        const ImxFramePose hd = cabinet_frame_pose(P, S, X, ft_cabinet_target(ft_off, n_ee, 0), B2, ec);
        s_fr[0 * 64 + lane] = tcp.px; s_fr[1 * 64 + lane] = tcp.py; s_fr[2 * 64 + lane] = tcp.pz;
        s_fr[3 * 64 + lane] = tcp.q.x; s_fr[4 * 64 + lane] = tcp.q.y; s_fr[5 * 64 + lane] = tcp.q.z; s_fr[6 * 64 + lane] = tcp.q.w;
        s_fr[7 * 64 + lane] = hd.px; s_fr[8 * 64 + lane] = hd.py; s_fr[9 * 64 + lane] = hd.pz;
        s_fr[10 * 64 + lane] = hd.q.x; s_fr[11 * 64 + lane] = hd.q.y; s_fr[12 * 64 + lane] = hd.q.z; s_fr[13 * 64 + lane] = hd.q.w;
        if (fingers) {
            const ImxFramePose lf = cabinet_frame_pose(P, S, X, ft_ee_target(ft_off, 1), B2, ec);
            const ImxFramePose rf = cabinet_frame_pose(P, S, X, ft_ee_target(ft_off, 2), B2, ec);
            s_fr[14 * 64 + lane] = lf.px; s_fr[15 * 64 + lane] = lf.py; s_fr[16 * 64 + lane] = lf.pz;
            s_fr[17 * 64 + lane] = rf.px; s_fr[18 * 64 + lane] = rf.py; s_fr[19 * 64 + lane] = rf.pz;
        }
    }
#endif

    // -- phase 0: everything that needs no table is issued at once: root state, and the episodic sum of this wave's first reward item
    const int first_rew = wv >= nterm ? wv - nterm : wv - nterm + ((nterm - wv + NW - 1) / NW) * NW;  // first item >= nterm of this wave
    const float es_first = (live && first_rew < nrew) ? Bf.episode_sums[(size_t)first_rew * N + e] : 0.0f;
    // slot t of the rollout storage (imx_terminations_rewards_rollout): what wave 0 needs at the very end is requested now
    const bool ro_on = ro.rewards_out != nullptr && wv == 0 && live;
    const float ro_value = ro_on ? ro.value_t[e] : 0.0f;
    const float ro_cur_rew = (ro_on && ro.cur_reward_sum) ? ro.cur_reward_sum[e] : 0.0f;
    const float ro_cur_len = (ro_on && ro.cur_ep_len) ? ro.cur_ep_len[e] : 0.0f;
    const float4 q4 = reinterpret_cast<const float4*>(S.root_quat_w)[ec];
    const float qw = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
    const float lwx = S.root_lin_vel_w[ec * 3], lwy = S.root_lin_vel_w[ec * 3 + 1], lwz = S.root_lin_vel_w[ec * 3 + 2];
    const float awx = S.root_ang_vel_w[ec * 3], awy = S.root_ang_vel_w[ec * 3 + 1], awz = S.root_ang_vel_w[ec * 3 + 2];
    const int64_t ep = Bf.episode_length_buf[ec] + 1;  // manager_based_rl_env.py:200
    const float cmdx = P.CMD > 0 ? S.command[ec * P.CMD + 0] : 0.0f;
    const float cmdy = P.CMD > 1 ? S.command[ec * P.CMD + 1] : 0.0f;
    const float cmdz = P.CMD > 2 ? S.command[ec * P.CMD + 2] : 0.0f;
    float lbx, lby, lbz, abx, aby, abz, pgx, pgy, pgz;
    quat_rotate_inverse(qw, qx, qy, qz, lwx, lwy, lwz, lbx, lby, lbz);
    quat_rotate_inverse(qw, qx, qy, qz, awx, awy, awz, abx, aby, abz);
    quat_rotate_inverse(qw, qx, qy, qz, P.gx, P.gy, P.gz, pgx, pgy, pgz);

    // -- the env's frame table for the observation kernel of the same step (what k_frame writes: same functions, same inputs, so
    //    bit-identical); the last wave has the fewest items
    if (frame && wv == NW - 1 && live) {
        float4 o[5];
        o[0] = make_float4(lbx, lby, lbz, abx);
        o[1] = make_float4(aby, abz, pgx, pgy);
        o[2] = make_float4(pgz, S.root_pos_w[e * 3], S.root_pos_w[e * 3 + 1], S.root_pos_w[e * 3 + 2]);
        o[3] = q4;
        o[4] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (P.R > 0 && P.ray_yaw_only) yaw_quat_wz(qw, qx, qy, qz, o[4].x, o[4].y);
        float4* dst = reinterpret_cast<float4*>(frame) + e * 6;
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[k] = o[k];
        if (P.R > 0 && !P.scan_stateful) dst[5] = make_float4(1.0f, o[2].y, o[2].z, o[2].w);  // a sensor without clock: cast, from the root
    }
    IMX_STAMP(1);
    IMX_STAMP(2);

    // -- phase 1: one item per trip.  TerminationManager.compute (termination_manager.py:151-174) / the reward functions
    const bool moving = sqrtf(cmdx * cmdx + cmdy * cmdy) > 0.1f;  // torch.norm(cmd[:, :2]) > 0.1
    for (int item = wv; item < nterm + nrew; item += NW) {
        if (item < nterm) {
            const int k = item;
            const int32_t* r = W + P.term_off + k * IMX_REC_WORDS;
            const int op = r[IMX_R_OP];
            const int n = r[IMX_R_NIDS];
            const int32_t* ids = W + (op == IMX_T_COMMAND_RESAMPLE ? 0 : r[IMX_R_IDS_OFF]);
            const float p0 = f_of(r[IMX_R_P0]), p1 = f_of(r[IMX_R_P1]);
            bool v = false;
            switch (op) {
                case IMX_T_TIME_OUT: v = ep >= (int64_t)P.max_ep_len; break;
                case IMX_T_ILLEGAL_CONTACT:
                    v = any_ids(ids, n, [&](int b) { return max_hist_force(S.net_forces_w_history, ec, H, Bn, b) > p0; });
                    break;
                case IMX_T_JOINT_POS_MANUAL_LIMIT:
                    v = any_ids(ids, n, [&](int j) { const float q = S.joint_pos[ec * J + j]; return (q > p1) || (q < p0); });
                    break;
                case IMX_T_BAD_ORIENTATION: v = fabsf(acosf(-pgz)) > p0; break;
#if defined(IMX_TR_LIFT) || defined(IMX_TR_INHAND)  // (the object's root only in these kernels: the launch sends such a plan there)
                case IMX_T_ROOT_HEIGHT_BELOW_MIN: v = (r[IMX_R_AUX0] ? S.object_root_pos_w : S.root_pos_w)[ec * 3 + 2] < p0; break;
#else
                case IMX_T_ROOT_HEIGHT_BELOW_MIN: v = S.root_pos_w[ec * 3 + 2] < p0; break;
#endif
                case IMX_T_JOINT_VEL_LIMIT:
                    v = any_ids(ids, n, [&](int j) { return fabsf(S.joint_vel[ec * J + j]) > S.soft_joint_vel_limits[ec * J + j]; });
                    break;
                case IMX_T_JOINT_VEL_MANUAL_LIMIT:
                    v = any_ids(ids, n, [&](int j) { return fabsf(S.joint_vel[ec * J + j]) > p0; });
                    break;
                case IMX_T_JOINT_EFFORT_LIMIT:  // torch.isclose(computed, applied): |a-b| <= atol + rtol*|b|
                    v = any_ids(ids, n, [&](int j) {
                        const float a = S.computed_torque[ec * J + j], b = S.applied_torque[ec * J + j];
                        return fabsf(a - b) <= 1.0e-8f + 1.0e-5f * fabsf(b);
                    });
                    break;
                case IMX_T_TERRAIN_OUT_OF_BOUNDS:
                    v = (fabsf(S.root_pos_w[ec * 3]) > p0) || (fabsf(S.root_pos_w[ec * 3 + 1]) > p1);
                    break;
                case IMX_T_EXTERNAL: v = S.ext_term[ec * (int64_t)P.w[IMX_H_NEXT_TERM] + r[IMX_R_AUX0]] != 0; break;
                case IMX_T_COMMAND_RESAMPLE:  // (time_left <= step_dt) & (command_counter == num_resamples)
                    v = (S.command_time_left[ec] <= p0) && (S.command_counter[ec] == (int64_t)n);
                    break;
#ifdef IMX_TR_LIFT
                case IMX_T_OBJECT_REACHED_GOAL: {  // lift/mdp/terminations.py:25-53 (the root quaternion and cmd[:3] of phase 0)
                        float px, py, pz;
                        command_des_pos_w(S.root_pos_w + ec * 3, q4, cmdx, cmdy, cmdz, px, py, pz);
                        v = object_goal_dist(S.object_root_pos_w + ec * 3, px, py, pz) < p0;
                    }
                    break;
#endif
#ifdef IMX_TR_INHAND  // inhand/mdp/terminations.py; cmdx, cmdy, cmdz = cmd[:3] of phase 0: the goal position in the env frame
                case IMX_T_MAX_CONSECUTIVE_SUCCESS: v = X.command_consecutive_success[ec] >= p0; break;  // :18-28
                case IMX_T_OBJECT_AWAY_FROM_GOAL: {  // :31-56: (object - origin) - goal, the norm as sqrt((x^2 + y^2) + z^2)
                        const float dx = (S.object_root_pos_w[ec * 3] - S.env_origins[ec * 3]) - cmdx;
                        const float dy = (S.object_root_pos_w[ec * 3 + 1] - S.env_origins[ec * 3 + 1]) - cmdy;
                        const float dz = (S.object_root_pos_w[ec * 3 + 2] - S.env_origins[ec * 3 + 2]) - cmdz;
                        v = sqrtf((dx * dx + dy * dy) + dz * dz) > p0;
                    }
                    break;
                case IMX_T_OBJECT_AWAY_FROM_ROBOT: {  // :59-83
                        const float dx = S.root_pos_w[ec * 3] - S.object_root_pos_w[ec * 3];
                        const float dy = S.root_pos_w[ec * 3 + 1] - S.object_root_pos_w[ec * 3 + 1];
                        const float dz = S.root_pos_w[ec * 3 + 2] - S.object_root_pos_w[ec * 3 + 2];
                        v = sqrtf((dx * dx + dy * dy) + dz * dz) > p0;
                    }
                    break;
#endif
                default: break;
            }
            s_tv[k * 64 + lane] = (v ? 1u : 0u) | (r[IMX_R_WEIGHT] ? 2u : 0u);  // bit 1: a time-out term (termination_manager.py:166-169)
            continue;
        }
        const int k = item - nterm;
        const int32_t* r = W + P.rew_off + k * IMX_REC_WORDS;
        const float es0 = k == first_rew ? es_first : (live ? Bf.episode_sums[(size_t)k * N + e] : 0.0f);
        float f = 0.0f;
        if (f_of(r[IMX_R_WEIGHT]) != 0.0f) {  // a zero-weight term is not evaluated (reward_manager.py:145)
            const int op = r[IMX_R_OP];
            const int n = r[IMX_R_NIDS];
            const int32_t* ids = W + r[IMX_R_IDS_OFF];
            const float p0 = f_of(r[IMX_R_P0]);
            switch (op) {
                // IS_ALIVE / IS_TERMINATED / IS_TERMINATED_TERM need the termination results: phase 2
                case IMX_W_LIN_VEL_Z_L2: f = lbz * lbz; break;
                case IMX_W_ANG_VEL_XY_L2: f = abx * abx + aby * aby; break;
                case IMX_W_FLAT_ORIENTATION_L2: f = pgx * pgx + pgy * pgy; break;
                case IMX_W_BASE_HEIGHT_L2: { const float d = S.root_pos_w[ec * 3 + 2] - p0; f = d * d; } break;
                case IMX_W_JOINT_TORQUES_L2:
                    f = sum_ids(ids, n, [&](int j) { const float x = S.applied_torque[ec * J + j]; return x * x; });
                    break;
                case IMX_W_JOINT_VEL_L1: f = sum_ids(ids, n, [&](int j) { return fabsf(S.joint_vel[ec * J + j]); }); break;
                case IMX_W_JOINT_VEL_L2:
                    f = sum_ids(ids, n, [&](int j) { const float x = S.joint_vel[ec * J + j]; return x * x; });
                    break;
                case IMX_W_JOINT_ACC_L2:
                    f = sum_ids(ids, n, [&](int j) { const float x = S.joint_acc[ec * J + j]; return x * x; });
                    break;
                case IMX_W_JOINT_DEVIATION_L1:
                    f = sum_ids(ids, n, [&](int j) { return fabsf(S.joint_pos[ec * J + j] - S.default_joint_pos[ec * J + j]); });
                    break;
                case IMX_W_JOINT_POS_LIMITS:
                    f = sum_ids(ids, n, [&](int j) {
                        const float q = S.joint_pos[ec * J + j];
                        const float2 lim = reinterpret_cast<const float2*>(S.soft_joint_pos_limits)[ec * J + j];
                        float o = -fminf(q - lim.x, 0.0f);
                        o += fmaxf(q - lim.y, 0.0f);
                        return o;
                    });
                    break;
                case IMX_W_JOINT_VEL_LIMITS:
                    f = sum_ids(ids, n, [&](int j) {
                        const float o = fabsf(S.joint_vel[ec * J + j]) - S.soft_joint_vel_limits[ec * J + j] * p0;
                        return fminf(fmaxf(o, 0.0f), 1.0f);
                    });
                    break;
                case IMX_W_APPLIED_TORQUE_LIMITS:
                    f = sum_ids(ids, n, [&](int j) { return fabsf(S.applied_torque[ec * J + j] - S.computed_torque[ec * J + j]); });
                    break;
                case IMX_W_ACTION_RATE_L2:
                    f = sum_range(A, [&](int i) { const float d = Bf.action[ec * A + i] - Bf.prev_action[ec * A + i]; return d * d; });
                    break;
                case IMX_W_ACTION_L2:
                    f = sum_range(A, [&](int i) { const float a = Bf.action[ec * A + i]; return a * a; });
                    break;
                case IMX_W_UNDESIRED_CONTACTS:
                    f = sum_ids(ids, n, [&](int b) { return (max_hist_force(S.net_forces_w_history, ec, H, Bn, b) > p0) ? 1.0f : 0.0f; });
                    break;
                case IMX_W_CONTACT_FORCES:
                    f = sum_ids(ids, n, [&](int b) { return fmaxf(max_hist_force(S.net_forces_w_history, ec, H, Bn, b) - p0, 0.0f); });
                    break;
                case IMX_W_TRACK_LIN_VEL_XY_EXP: {
                    const float ex = cmdx - lbx, ey = cmdy - lby;
                    f = expf(-(ex * ex + ey * ey) / p0);  // p0 = std**2
                } break;
                case IMX_W_TRACK_ANG_VEL_Z_EXP: { const float ez = cmdz - abz; f = expf(-(ez * ez) / p0); } break;
                case IMX_W_FEET_AIR_TIME: {
                    // first_contact = (cct > 0) * (cct < dt + abs_tol); p1 = float32(step_dt + 1e-8)
                    const float p1 = f_of(r[IMX_R_P1]);
                    f = sum_ids(ids, n, [&](int b) {
                        const float cct = S.current_contact_time[ec * Bn + b];
                        const float fc = (cct > 0.0f && cct < p1) ? 1.0f : 0.0f;
                        return (S.last_air_time[ec * Bn + b] - p0) * fc;
                    });
                    f *= moving ? 1.0f : 0.0f;
                } break;
                case IMX_W_FEET_AIR_TIME_POSITIVE_BIPED: {
                    int n_contact = 0;
                    float mn = __builtin_huge_valf();
                    for (int i = 0; i < n; ++i) n_contact += (S.current_contact_time[ec * Bn + ids[i]] > 0.0f) ? 1 : 0;
                    for (int i = 0; i < n; ++i) {
                        const float ct = S.current_contact_time[ec * Bn + ids[i]], at = S.current_air_time[ec * Bn + ids[i]];
                        const float in_mode = (ct > 0.0f) ? ct : at;
                        mn = fminf(mn, (n_contact == 1) ? in_mode : 0.0f);
                    }
                    f = fminf(mn, p0);
                    f *= moving ? 1.0f : 0.0f;
                } break;
                case IMX_W_FEET_SLIDE: {
                    const int32_t* ids2 = W + r[IMX_R_IDS2_OFF];
                    for (int i = 0; i < n; ++i) {
                        const float c = (max_hist_force(S.net_forces_w_history, ec, H, Bn, ids[i]) > 1.0f) ? 1.0f : 0.0f;
                        const float* v = S.body_lin_vel_w + ((size_t)ec * P.NB + ids2[i]) * 3;
                        f += sqrtf(v[0] * v[0] + v[1] * v[1]) * c;
                    }
                } break;
                case IMX_W_TRACK_LIN_VEL_XY_YAW_FRAME_EXP: {
                    float yw, yz, vx, vy, vz;
                    yaw_quat_wz(qw, qx, qy, qz, yw, yz);
                    quat_rotate_inverse(yw, 0.0f, 0.0f, yz, lwx, lwy, lwz, vx, vy, vz);
                    const float ex = cmdx - vx, ey = cmdy - vy;
                    f = expf(-(ex * ex + ey * ey) / p0);
                } break;
                case IMX_W_TRACK_ANG_VEL_Z_WORLD_EXP: { const float ez = cmdz - awz; f = expf(-(ez * ez) / p0); } break;
                case IMX_W_JOINT_POS_TARGET_L2:
                    f = sum_ids(ids, n, [&](int j) { const float d = wrap_to_pi(S.joint_pos[ec * J + j]) - p0; return d * d; });
                    break;
                case IMX_W_EXTERNAL: f = S.ext_reward[ec * (int64_t)P.w[IMX_H_NEXT_REW] + r[IMX_R_AUX0]]; break;
                case IMX_W_BODY_LIN_ACC_L2:  // sum over bodies of ||body_lin_acc_w|| (rewards.py:125-128)
                    f = sum_ids(ids, n, [&](int b) {
                        const float* a = S.body_lin_acc_w + ((size_t)ec * P.NB + b) * 3;
                        return norm3(a[0], a[1], a[2]);
                    });
                    break;
                // ---- Spot (isaaclab_tasks .../velocity/config/spot/mdp/rewards.py).  "active" = torch.logical_or(||cmd|| > 0,
                //      ||v_b,xy|| > velocity_threshold) with the norm of the WHOLE command, yaw rate included (:52-53, :150-151, :264-268)
                case IMX_W_AIR_TIME_REWARD: {  // :31-58, ids = the 4 feet of the sensor
                    const bool act = spot_active(cmdx, cmdy, cmdz, lbx, lby, f_of(r[IMX_R_P1]));
                    f = sum_ids(ids, n, [&](int b) {
                        const float at = S.current_air_time[ec * Bn + b], ct = S.current_contact_time[ec * Bn + b];
                        const float t_max = fmaxf(at, ct);
                        const float stance = fminf(fmaxf(ct - at, -p0), p0);  // clip(contact - air, -mode_time, mode_time)
                        return act ? (t_max < p0 ? fminf(t_max, p0) : 0.0f) : stance;
                    });
                } break;
                case IMX_W_BASE_ANGULAR_VELOCITY_REWARD: f = expf(-fabsf(cmdz - abz) / p0); break;  // :61-68
                case IMX_W_BASE_LINEAR_VELOCITY_REWARD: {  // :71-83
                    const float ex = cmdx - lbx, ey = cmdy - lby;
                    const float err = sqrtf(ex * ex + ey * ey), mag = sqrtf(cmdx * cmdx + cmdy * cmdy);
                    const float mult = fmaxf(1.0f + f_of(r[IMX_R_P1]) * (mag - f_of(r[IMX_R_P2])), 1.0f);
                    f = expf(-err / p0) * mult;
                } break;
                case IMX_W_GAIT_REWARD: {  // :86-177, ids = pair0[0], pair0[1], pair1[0], pair1[1]; p1 = max_err**2
                    const float p1 = f_of(r[IMX_R_P1]);
                    float at[4], ct[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        at[u] = S.current_air_time[ec * Bn + ids[u]];
                        ct[u] = S.current_contact_time[ec * Bn + ids[u]];
                    }
                    auto pair_reward = [&](float a0, float a1, float c0, float c1) {  // exp(-(clip(d1^2) + clip(d2^2)) / std)
                        const float d1 = a0 - a1, d2 = c0 - c1;
                        return expf(-(fminf(d1 * d1, p1) + fminf(d2 * d2, p1)) / p0);
                    };
                    const float sync = pair_reward(at[0], at[1], ct[0], ct[1]) * pair_reward(at[2], at[3], ct[2], ct[3]);
                    // _async_reward_func(f0, f1): air(f0) against contact(f1), contact(f0) against air(f1)
                    const float async = pair_reward(at[0], ct[2], ct[0], at[2]) * pair_reward(at[1], ct[3], ct[1], at[3]) *
                                        pair_reward(at[0], ct[3], ct[0], at[3]) * pair_reward(at[2], ct[1], ct[2], at[1]);
                    f = spot_active(cmdx, cmdy, cmdz, lbx, lby, f_of(r[IMX_R_P2])) ? sync * async : 0.0f;
                } break;
                case IMX_W_FOOT_CLEARANCE_REWARD: {  // :180-188, ids = asset bodies; the only reader of body_pos_w
                    const float p1 = f_of(r[IMX_R_P1]), p2 = f_of(r[IMX_R_P2]);
                    const float s = sum_ids(ids, n, [&](int b) {
                        const size_t o = ((size_t)ec * P.NB + b) * 3;
                        const float dz = S.body_pos_w[o + 2] - p0;
                        const float vx = S.body_lin_vel_w[o], vy = S.body_lin_vel_w[o + 1];
                        return (dz * dz) * tanhf(p2 * sqrtf(vx * vx + vy * vy));
                    });
                    f = expf(-s / p1);
                } break;
                case IMX_W_ACTION_SMOOTHNESS_PENALTY:  // :196-198, the norm, not its square
                    f = sqrtf(sum_range(A, [&](int i) { const float d = Bf.action[ec * A + i] - Bf.prev_action[ec * A + i]; return d * d; }));
                    break;
                case IMX_W_AIR_TIME_VARIANCE_PENALTY: {  // :201-212, torch.var: unbiased (divisor n - 1) of the times clipped at 0.5
                    auto var_clipped = [&](const float* __restrict__ t) {
                        const float mean = sum_ids(ids, n, [&](int b) { return fminf(t[ec * Bn + b], 0.5f); }) / (float)n;
                        const float ss = sum_ids(ids, n, [&](int b) { const float d = fminf(t[ec * Bn + b], 0.5f) - mean; return d * d; });
                        return ss / (float)(n - 1);
                    };
                    f = var_clipped(S.last_air_time) + var_clipped(S.last_contact_time);
                } break;
                case IMX_W_BASE_MOTION_PENALTY: f = 0.8f * (lbz * lbz) + 0.2f * (fabsf(abx) + fabsf(aby)); break;  // :216-222
                case IMX_W_BASE_ORIENTATION_PENALTY: f = sqrtf(pgx * pgx + pgy * pgy); break;                     // :225-232
                case IMX_W_FOOT_SLIP_PENALTY: {  // :235-249, ids = sensor bodies, ids2 = asset bodies, p0 = threshold
                    const int32_t* ids2 = W + r[IMX_R_IDS2_OFF];
                    for (int i = 0; i < n; ++i) {
                        const float c = (max_hist_force(S.net_forces_w_history, ec, H, Bn, ids[i]) > p0) ? 1.0f : 0.0f;
                        const float* v = S.body_lin_vel_w + ((size_t)ec * P.NB + ids2[i]) * 3;
                        f += c * sqrtf(v[0] * v[0] + v[1] * v[1]);
                    }
                } break;
                case IMX_W_JOINT_ACCELERATION_PENALTY:  // :252-256 (ids = every joint)
                    f = sqrtf(sum_ids(ids, n, [&](int j) { const float x = S.joint_acc[ec * J + j]; return x * x; }));
                    break;
                case IMX_W_JOINT_POSITION_PENALTY: {  // :259-268, p0 = stand_still_scale, p1 = velocity_threshold
                    const float d = sqrtf(sum_ids(ids, n, [&](int j) {
                        const float x = S.joint_pos[ec * J + j] - S.default_joint_pos[ec * J + j];
                        return x * x;
                    }));
                    f = spot_active(cmdx, cmdy, cmdz, lbx, lby, f_of(r[IMX_R_P1])) ? d : p0 * d;
                } break;
                case IMX_W_JOINT_TORQUES_PENALTY:  // :271-275
                    f = sqrtf(sum_ids(ids, n, [&](int j) { const float x = S.applied_torque[ec * J + j]; return x * x; }));
                    break;
                case IMX_W_JOINT_VELOCITY_PENALTY:  // :278-282
                    f = sqrtf(sum_ids(ids, n, [&](int j) { const float x = S.joint_vel[ec * J + j]; return x * x; }));
                    break;
                default: break;
            }
        }
        s_f[k * 64 + lane] = f;
        s_es[k * 64 + lane] = es0;
    }
    IMX_STAMP(3);
    __syncthreads();
    IMX_STAMP(4);

    // -- phase 2: every termination is known
    uint32_t term_bits = 0u, trunc_mask = 0u;
    for (int k = 0; k < nterm; ++k) {
        const uint32_t x = s_tv[k * 64 + lane];
        term_bits |= (x & 1u) << k;
        trunc_mask |= ((x >> 1) & 1u) << k;
    }
    const bool truncated = (term_bits & trunc_mask) != 0u, terminated = (term_bits & ~trunc_mask) != 0u;
    const bool reset = live && (terminated || truncated);
    if (frame && P.scan_stateful && wv == NW - 1 && live) {  // the sensor's clock, now that the env's reset flag is known (scene.reset(env_ids))
        reinterpret_cast<float4*>(frame)[e * 6 + 5] =
            scanner_step(P, Bf, e, step, reset, S.root_pos_w[e * 3], S.root_pos_w[e * 3 + 1], S.root_pos_w[e * 3 + 2]);
    }
    // RewardManager.compute (reward_manager.py:128-157): value = f * w * dt; sums += value; step_reward = value/dt
    const float dt = P.step_dt;
    for (int k = wv; k < nrew; k += NW) {
        const int32_t* r = W + P.rew_off + k * IMX_REC_WORDS;
        const float weight = f_of(r[IMX_R_WEIGHT]);
        const float es0 = s_es[k * 64 + lane];
        float es = es0, value = 0.0f;
        if (weight != 0.0f) {
            float f = s_f[k * 64 + lane];
            const int op = r[IMX_R_OP];
            if (op == IMX_W_IS_ALIVE) f = terminated ? 0.0f : 1.0f;
            if (op == IMX_W_IS_TERMINATED) f = terminated ? 1.0f : 0.0f;
            if (op == IMX_W_IS_TERMINATED_TERM) {
                const int n = r[IMX_R_NIDS];
                const int32_t* ids = W + r[IMX_R_IDS_OFF];
                float sum = 0.0f;
                for (int i = 0; i < n; ++i) sum += ((term_bits >> ids[i]) & 1u) ? 1.0f : 0.0f;
                f = sum * (truncated ? 0.0f : 1.0f);
            }
            if (CLASSIC && op >= IMX_W_UPRIGHT_POSTURE_BONUS) f = classic_reward(P, S, Bf, r, op, live ? e : min(grp * G, N - 1), N);
#ifdef IMX_TR_NAV
            if (op >= IMX_W_NAV_POSITION_COMMAND_ERROR_TANH) f = nav_reward(P, S, r, op, live ? e : min(grp * G, N - 1));
#endif
#ifdef IMX_TR_INHAND
            if (op >= IMX_W_TRACK_ORIENTATION_INV_L2) f = inhand_reward(P, S, r, op, live ? e : min(grp * G, N - 1), s_dth[lane]);
#endif
#ifdef IMX_TR_CABINET
            if (op >= IMX_W_APPROACH_EE_HANDLE) f = cabinet_reward(P, S, X, r, op, live ? e : min(grp * G, N - 1), s_fr + lane, W[ft_off]);
#endif
#ifdef IMX_TR_LIFT
            if (op >= IMX_W_POSITION_COMMAND_ERROR && op < IMX_W_OBJECT_IS_LIFTED) f = reach_reward(P, S, r, op, live ? e : min(grp * G, N - 1));
            if (op >= IMX_W_OBJECT_IS_LIFTED) f = lift_reward(P, S, r, op, live ? e : min(grp * G, N - 1));
#else
            if (REACH && op >= IMX_W_POSITION_COMMAND_ERROR) f = reach_reward(P, S, r, op, live ? e : min(grp * G, N - 1));
#endif
            value = f * weight * dt;
            es = es0 + value;
            if (live) Bf.step_reward[(size_t)e * nrew + k] = value / dt;
        }
        // (a skipped term leaves step_reward as it was and still takes part in the reset / log pass, reward_manager.py:100-126,145)
        if (CLASSIC && r[IMX_R_OP] == IMX_W_PROGRESS_REWARD && live && (weight != 0.0f || reset)) {
            // potentials after the step: __call__'s value (a zero-weight term is not called), then RewardManager.reset -> progress_reward.
            // reset (rewards.py:54-60) for a reset env: the 3-D distance of this step's root position
            const float tx = f_of(r[IMX_R_P0]), ty = f_of(r[IMX_R_P1]), tz = f_of(r[IMX_R_P2]);
            Bf.term_state[(size_t)r[IMX_R_AUX0] * N + e] =
                progress_potential(tx, ty, tz, S.root_pos_w[e * 3], S.root_pos_w[e * 3 + 1], S.root_pos_w[e * 3 + 2], dt, reset);
        }
        s_val[k * 64 + lane] = value;
        if (live && (weight != 0.0f || reset)) Bf.episode_sums[(size_t)k * N + e] = reset ? 0.0f : es;
        // RewardManager.reset log (reward_manager.py:115-121): mean over reset envs of the episodic sum
        const float part = wave_sum(reset ? es : 0.0f);
        if (lane == 0) sc.log_part[grp * nrew + k] = part;
    }
    // termination bookkeeping by the waves from the far end (wave 0 is busy below)
    for (int k = NW - 1 - wv; k < nterm; k += NW) {
        const bool v = (term_bits >> k) & 1u;
        if (live) Bf.term_dones[(size_t)k * N + e] = v ? 1 : 0;
        // TerminationManager.reset log (termination_manager.py:142-144): count_nonzero(term_dones[reset ids])
        const int c = wave_sum_i((reset && v) ? 1 : 0);
        if (lane == 0) sc.term_part[grp * nterm + k] = c;
    }
    IMX_STAMP(5);
    __syncthreads();
    IMX_STAMP(6);

    // -- phase 3
    if (wv == 0) {
        float reward = 0.0f;
        for (int k = 0; k < nrew; ++k) reward += s_val[k * 64 + lane];  // term order (a skipped term holds +0: x + 0 == x bit for bit)
        // -- outputs + manager-side _reset_idx (manager_based_rl_env.py:347-392)
        if (live) {
            Bf.reward_buf[e] = reward;
            Bf.terminated[e] = terminated ? 1 : 0;
            Bf.truncated[e] = truncated ? 1 : 0;
            Bf.reset_buf[e] = reset ? 1 : 0;
            Bf.episode_length_buf[e] = reset ? 0 : ep;
            if (reset)
                for (int i = 0; i < A; ++i) {  // ActionManager.reset (action_manager.py:306-316)
                    Bf.action[e * A + i] = 0.0f;
                    Bf.prev_action[e * A + i] = 0.0f;
                }
        }
        // slot t of the RolloutStorage (what imx_rollout_post does in a launch of its own): RslRlVecEnvWrapper.step's dones
        // (vecenv_wrapper.py:178), PPO.process_env_step's time-out bootstrap, the runner's episode book-keeping -- same expressions,
        // bit-identical
        if (ro.rewards_out) {
            float s_r = 0.0f, s_l = 0.0f, s_c = 0.0f;
            if (live) {
                ro.rewards_out[e] = ro.bootstrap_time_outs ? reward + ro.gamma * (ro_value * (truncated ? 1.0f : 0.0f)) : reward;
                ro.dones_out[e] = reset ? 1 : 0;
                if (ro.cur_reward_sum) {
                    const float cr = ro_cur_rew + reward, cl = ro_cur_len + 1.0f;
                    if (reset) { s_r = cr; s_l = cl; s_c = 1.0f; }
                    ro.cur_reward_sum[e] = reset ? 0.0f : cr;
                    ro.cur_ep_len[e] = reset ? 0.0f : cl;
                }
            }
            if (ro.ep_stats3) {
                s_r = wave_sum(s_r); s_l = wave_sum(s_l); s_c = wave_sum(s_c);
                if (lane == 0 && s_c > 0.0f) {
                    atomicAdd(&ro.ep_stats3[0], s_r); atomicAdd(&ro.ep_stats3[1], s_l); atomicAdd(&ro.ep_stats3[2], s_c);
                }
            }
        }
        // ordered compaction inside the group: reset_env_ids = reset_buf.nonzero() (manager_based_rl_env.py:215)
        const unsigned long long ballot = __ballot(reset);
        const int before = __popcll(ballot & ((1ull << lane) - 1ull));
        if (reset) sc.ids_local[grp * 64 + before] = lane;
        if (lane == 0) sc.wave_cnt[grp] = __popcll(ballot);
    }

    IMX_STAMP(7);
    if (defer_tail) return;  // imx_observations of the same step finishes (step_tail in an extra workgroup of k_obs)
    // producer side (cdna_hip_programming.md G16, R1): every storing wave drains its stores, the block meets at the
    // barrier, ONE lane releases at agent scope and takes the ticket
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int ticket = atomicAdd(&Bf.counters[1], 1);
        s_last = (ticket == (int)gridDim.x - 1);
        if (s_last) {  // consumer side: one agent-scope acquire, completed before the barrier releases the readers
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            Bf.counters[1] = 0;  // re-arm the ticket
        }
    }
    __syncthreads();
    if (!s_last) return;
    step_tail(P, N, Bf, sc, G, 0, 1);
