// The body of k_obs (step.hip), included once per kernel: in k_obs<GENERAL_RAYS, LEAN> as it always was, and in k_obs_inhand<LEAN>
// with IMX_OBS_INHAND defined (the root observations on the scene's rigid object, goal_quat_diff: obs_inhand_value), in
// k_obs_cabinet<LEAN> with IMX_OBS_CABINET (the FrameTransformer frames, the second articulation's joints: obs_cabinet_value).  A textual include like
// term_rew_body.inc, for the same reason: the kernels of the existing tasks compile to the very instruction streams they had.
    // One workgroup per env.  (A resident grid walking the envs -- sized to what the chip holds at once -- was measured and dropped:
    // the loop costs 13 more VGPRs, i.e. one wave per SIMD less, and three uneven rounds: 35 us against 29.)
    if ((int)blockIdx.x < tail_parts) {  // extra workgroups, first in the grid: the step tail k_term_rew deferred (kernel boundary = its partials are complete)
        step_tail(P, N, Bf, sc, tail_G, (int)blockIdx.x, tail_parts);
        return;
    }
    const int64_t e = blockIdx.x - (unsigned)tail_parts;
    const int32_t* __restrict__ W = P.w;
    const uint32_t step = (uint32_t)Bf.counters[2];
    const bool fill_all = (corrupt & 2) != 0;
    const bool keep_all_hits = (corrupt & 8) != 0;
    corrupt &= 1;
    extern __shared__ float s_hz[];  // R hit heights of this env
    const float* __restrict__ es = frame + e * IMX_ES_WORDS;  // wave-uniform address
    const float yw = es[16], yz = es[17];
    // the sensor's decision for this step (scanner_step, made where the frame row was produced): cast?  keep the hits?  from where?
    const int sflags = (int)es[20];
    const bool cast = (sflags & 1) != 0, cache_z = P.scan_stateful && ((sflags & 2) || keep_all_hits);
    const float px = es[21], py = es[22], pz = es[23];
#ifdef IMX_TRACE
    const uint64_t trace_tp = 0;
    const uint64_t trace_t0 = wall_clock64();
    uint64_t trace_t1 = 0, trace_t2 = 0;
#endif
    // -- phase A: the env's rays.  RayCaster._update_buffers_impl (ray_caster.py:242-260): ray j of the scanner -> hit height into LDS.
    //    Kept apart from the column loop below on purpose: what limits this kernel is how many waves a SIMD can hold (wave life x
    //    residency, tools/trace_kobs.py), i.e. its register count -- a ray lane carries the ray and one cell's data, a column lane its
    //    16-word column record, never both.
    if (P.R > 0) {
        const float* __restrict__ ray_local = reinterpret_cast<const float*>(W + P.ray_off);
        for (int j = threadIdx.x; j < P.R; j += blockDim.x) {
            float hz;
            if (cast) {
                hz = scan_ray<GENERAL_RAYS>(P, M, es, ray_local, j, px, py, pz, yw, yz, ray_hits_out, e);
                if (cache_z) Bf.scan_hit_z[(size_t)e * P.R + j] = hz;
            } else {
                hz = Bf.scan_hit_z[(size_t)e * P.R + j];  // data.ray_hits_w of the last update
            }
            s_hz[j] = hz;
        }
#ifdef IMX_TRACE
        trace_t1 = wall_clock64();
#endif
        __syncthreads();
#ifdef IMX_TRACE
        trace_t2 = wall_clock64();
#endif
    }
    if (e == 0 && threadIdx.x == 0) Bf.counters[3] = (int32_t)step;  // the shadow the next step kernel counts on from
    // -- phase B: the observation columns (ObservationManager.compute_group, observation_manager.py:260-335)
    for (int i = threadIdx.x; i < P.DC; i += blockDim.x) {
        const XCol x = load_xcol(W, P.xcol_off, i);
        const int op = x.a.y, j = x.a.z;
        float v;
        if (op == IMX_O_HEIGHT_SCAN) {  // height_scan (observations.py:165-173): sensor.data.pos_w z - hit z - offset
            const float hz = s_hz[j];
            v = pz - hz - f_of(x.b.x);
            // further height_scan terms on the same sensor (another group, another offset / noise / clip): same hit, own post-processing
            for (int nx = LEAN ? 0 : x.c.z; nx != 0;) {
                const XCol tw = load_xcol(W, P.xcol_off, nx - 1);
                obs_finish<false>(P, Bf, tw, nx - 1, pz - hz - f_of(tw.b.x), e, corrupt, fill_all, noise_u, seed, step);
                nx = tw.c.z;
            }
        } else {
#if defined(IMX_OBS_INHAND)
            v = obs_inhand_value(P, S, X, Bf, es, e, x);
#elif defined(IMX_OBS_CABINET)
            v = obs_cabinet_value(P, S, X, Bf, es, e, x);
#elif defined(IMX_OBS_IMU)
            v = obs_imu_value(P, S, X, Bf, es, e, x);
#else
            v = obs_plain_value<true>(P, S, Bf, es, e, x);
#endif
        }
        obs_finish<LEAN>(P, Bf, x, i, v, e, corrupt, fill_all, noise_u, seed, step);
    }
#ifdef IMX_TRACE
    if (g_trace && (threadIdx.x & 63) == 0) {
        uint64_t* t = g_trace + ((size_t)e * 4 + (threadIdx.x >> 6)) * 8;
        t[0] = trace_t0; t[1] = wall_clock64();
        t[2] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_ID (wave/simd/cu/sh/se ids)
        t[3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));   // XCC_ID
        t[4] = trace_t1; t[5] = trace_t2; t[6] = trace_tp;
    }
#endif
