// PreTrainedPolicyAction (isaaclab_tasks .../navigation/mdp/pre_trained_policy_action.py:93-100): one low-level locomotion step for all
// envs in ONE launch -- imx_pretrained_policy.
//
// A workgroup owns ROWS (16 or 32) envs and walks the four stages the reference runs as ~40 eager launches, and the existing kernels
// as a chain of four (k_frame, k_obs, k_mlp_infer16 / k_mlp_infer, k_action):
//   0  the root-frame vectors of its rows (k_frame's arithmetic, one lane per row) -> LDS
//   1  every observation column of every row, through the device functions of the observation kernels (obs_plain_value, obs_post:
//      value, noise draw keyed by (seed, step, env * D + column), clip, scale), straight into the LDS input tile of the MFMA layers
//      (no (N, D) round trip through memory); a last_action column of an env whose episode_length_buf is 0 reads 0 -- the masked
//      zero of the term's last_action() closure (:53-57), whose write to low_level_actions stage 3 overwrites anyway
//   2  the Linear + ELU layers on the MFMA (infer_layer16 / infer_layer, activations ping-pong in LDS), the output kept in LDS
//   3  lane = (row, action column): action_process_element on the low-level plan: low_level_actions <- the policy output, the joint
//      position targets <- raw * scale + offset [clip]
// Same device functions, same summation order as the chain: bit-identical to it when its imx_mlp_infer runs the same tile height.
#include "imx_internal.h"
#include "imx_obs_device.h"
#include "imx_infer_device.h"

#define IMX_PP_ES 16  // floats of a row's frame: 0-2 lin vel b, 3-5 ang vel b, 6-8 projected gravity, 9-11 root pos, 12-15 root quat

struct PolicyArgs {
    int64_t N;
    const float* W[IMX_PP_MAX_LAYERS];   // the row layout, or the packed image for the 32-row kernel
    const float* b[IMX_PP_MAX_LAYERS];
    int ldw[IMX_PP_MAX_LAYERS];
    int dim[IMX_PP_MAX_LAYERS + 1];
    int nlayers;
    float alpha;
    const float* noise_u;
    uint64_t seed;
    const int32_t* step_d;
    int step_stride, step_offset;
    int corrupt;
    float* obs_out;
};

template <int ROWS, bool PACKED>
__global__ void __launch_bounds__(256, ROWS == 16 ? 2 : 1)
k_pretrained_policy(PlanView P, imx_state_t S, imx_buffers_t Bf, PolicyArgs a) {
    extern __shared__ float smem[];  // two activation buffers of ROWS x INF_PITCH floats, then ROWS frames
    float* buf0 = smem;
    float* buf1 = smem + ROWS * INF_PITCH;
    float* es_s = smem + 2 * ROWS * INF_PITCH;
    const int64_t m0 = (int64_t)blockIdx.x * ROWS, N = a.N;
    const int D = P.gD[0], K0p = (D + 31) & ~31;
    const uint32_t step = (uint32_t)((a.step_d ? a.step_d[0] : 0) * a.step_stride + a.step_offset);
    // -- stage 0: k_frame's vectors for the rows of the tile (rows past N: zeros, never read)
    if (threadIdx.x < ROWS) {
        const int64_t e = m0 + threadIdx.x;
        float* o = es_s + threadIdx.x * IMX_PP_ES;
        if (e < N) {
            const float4 q4 = reinterpret_cast<const float4*>(S.root_quat_w)[e];
            quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, S.root_lin_vel_w[e * 3], S.root_lin_vel_w[e * 3 + 1], S.root_lin_vel_w[e * 3 + 2],
                                o[0], o[1], o[2]);
            quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, S.root_ang_vel_w[e * 3], S.root_ang_vel_w[e * 3 + 1], S.root_ang_vel_w[e * 3 + 2],
                                o[3], o[4], o[5]);
            quat_rotate_inverse(q4.x, q4.y, q4.z, q4.w, P.gx, P.gy, P.gz, o[6], o[7], o[8]);
            o[9] = S.root_pos_w[e * 3]; o[10] = S.root_pos_w[e * 3 + 1]; o[11] = S.root_pos_w[e * 3 + 2];
            o[12] = q4.x; o[13] = q4.y; o[14] = q4.z; o[15] = q4.w;
        } else {
#pragma unroll
            for (int k = 0; k < IMX_PP_ES; ++k) o[k] = 0.0f;
        }
    }
    // the padding columns [D, K0p) the first layer's 32-wide reduction groups read
    for (int i = threadIdx.x; i < ROWS * (K0p - D); i += blockDim.x) {
        const int row = i / (K0p - D), col = D + i - row * (K0p - D);
        buf0[row * INF_PITCH + col] = 0.0f;
    }
    __syncthreads();
    // -- stage 1: the observation rows (ObservationManager.compute_group, observation_manager.py:260-335) into the input tile.
    //    Consecutive lanes take consecutive computed columns of one row (the host admits plans with DC == D == gD[0] only).
    for (int i = threadIdx.x; i < ROWS * D; i += blockDim.x) {
        const int row = i / D, ci = i - row * D;
        const int64_t e = m0 + row;
        const XCol x = load_xcol(P.w, P.xcol_off, ci);
        float v = 0.0f;
        if (e < N) {
            v = obs_plain_value<false>(P, S, Bf, es_s + row * IMX_PP_ES, e, x);
            if (x.a.y == IMX_O_LAST_ACTION && Bf.episode_length_buf[e] == 0) v = 0.0f;  // last_action() :53-57
            v = obs_post<true>(x, v, a.corrupt & P.gcorrupt, a.noise_u, a.seed, step, e, P.D, 0);
            if (a.obs_out) a.obs_out[e * D + x.a.x] = v;
        }
        buf0[row * INF_PITCH + x.a.x] = v;
    }
    __syncthreads();
    // -- stage 2: the layers (the rollout inference kernels' loop; the last layer's output stays in LDS)
    const float* in = infer_layers<ROWS, PACKED>(buf0, buf1, a, a.W, true, [] { return (float*)nullptr; }, m0, N).in;
    // -- stage 3: low_level_actions[:] = policy(obs); JointPositionAction.process_actions (joint_actions.py:130-139)
    const int A = P.A;
    for (int i = threadIdx.x; i < ROWS * A; i += blockDim.x) {
        const int row = i / A, c = i - row * A;
        const int64_t e = m0 + row;
        if (e < N) action_process_element<false>(P, S, Bf, e, c, in[row * INF_PITCH + c], __builtin_huge_valf());
    }
}

static int g_pp_num_cu = 0;
static int pp_num_cu() {
    if (g_pp_num_cu == 0) {
        int dev = 0, cu = 0;  // (as imx_mlp_infer counts them)
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0)
            cu = 256;
        g_pp_num_cu = cu;
    }
    return g_pp_num_cu;
}

// imx_mlp_infer's rule for one network: 16-row tiles when 32-row tiles would leave at least half of the CUs without a workgroup
extern "C" int imx_pretrained_policy_tile_rows(int64_t N) {
    const int64_t tiles32 = (N + 31) / 32;
    return tiles32 * 2 <= pp_num_cu() ? 16 : 32;
}

static bool pp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Everything that can be refused without a device: the arguments, the plan's shape, the policy's shape, the state tensors the records read.
static int pp_check(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf, const imx_pretrained_policy_t* pol,
                    int tile_rows) {
    IMX_REQUIRE(plan && st && bf && pol, "imx_pretrained_policy: null plan / state / buffers / policy");
    IMX_REQUIRE(N >= 1 && N < (1ll << 31), "imx_pretrained_policy: num_envs out of range: %lld", (long long)N);
    IMX_REQUIRE(tile_rows == 0 || tile_rows == 16 || tile_rows == 32, "imx_pretrained_policy: tile_rows %d (0, 16 or 32)", tile_rows);
    IMX_REQUIRE(plan->ngroups == 1 && plan->MS == 0 && plan->DC == plan->D && plan->DX == plan->DC && plan->R == 0 && plan->D == plan->gD[0],
                "imx_pretrained_policy: the low-level plan must hold one observation group without history, modifiers or a height scan");
    IMX_REQUIRE(pol->nlayers >= 1 && pol->nlayers <= IMX_PP_MAX_LAYERS, "imx_pretrained_policy: %d layers (1..%d supported)", pol->nlayers,
                IMX_PP_MAX_LAYERS);
    for (int l = 0; l <= pol->nlayers; ++l)
        IMX_REQUIRE(pol->dims[l] >= 1 && pol->dims[l] <= INF_MAXD, "imx_pretrained_policy: layer width %d outside 1..%d", pol->dims[l], INF_MAXD);
    IMX_REQUIRE(pol->dims[0] == plan->D, "imx_pretrained_policy: the policy takes %d inputs, the low-level observation group has %d columns",
                pol->dims[0], plan->D);
    IMX_REQUIRE(pol->dims[pol->nlayers] == plan->A && plan->A > 0, "imx_pretrained_policy: the policy has %d outputs, the low-level action term %d columns",
                pol->dims[pol->nlayers], plan->A);
    IMX_REQUIRE(plan->PA == plan->A, "imx_pretrained_policy: a low-level action term whose processed width differs from its raw width");
    bool packed = pol->packed_weights_d[0] != nullptr;
    for (int l = 0; l < pol->nlayers; ++l) {
        IMX_REQUIRE(pol->weights_d[l] && pol->biases_d[l], "imx_pretrained_policy: null weight / bias (layer %d)", l);
        IMX_REQUIRE(pol->weight_pitch[l] >= pol->dims[l] && pol->weight_pitch[l] % 32 == 0 && pp_aligned16(pol->weights_d[l]),
                    "imx_pretrained_policy: weights of layer %d need a 16-byte aligned, zero-padded row pitch that is a multiple of 32 floats "
                    "(pitch %d, in-features %d)", l, pol->weight_pitch[l], pol->dims[l]);
        IMX_REQUIRE((pol->packed_weights_d[l] != nullptr) == packed && pp_aligned16(pol->packed_weights_d[l]),
                    "imx_pretrained_policy: packed weights must be given for every layer or for none, 16-byte aligned (layer %d)", l);
    }
    IMX_REQUIRE(st->root_quat_w && st->root_lin_vel_w && st->root_ang_vel_w && st->root_pos_w, "imx_pretrained_policy: root state missing");
    IMX_REQUIRE(bf->episode_length_buf, "imx_pretrained_policy: null episode_length_buf");
    const auto& w = plan->host;
    for (int k = 0; k < plan->nobs; ++k) {
        const int op = w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_OP];
        IMX_REQUIRE(!(w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_FLAGS] & IMX_F_MODIFIERS), "imx_pretrained_policy: observation record %d has modifiers", k);
        const void* p = (const void*)1;
        const char* name = "";
        if (op >= IMX_O_ROOT_POS_W && op <= IMX_O_ROOT_ANG_VEL_W && w[plan->obs_off + k * IMX_REC_WORDS + IMX_R_AUX0])
            IMX_FAIL("imx_pretrained_policy: observation record %d (op %d on the rigid object) is not built into the fused low-level step", k, op);
        switch (op) {
            case IMX_O_ROOT_POS_W: p = st->env_origins; name = "env_origins"; break;
            case IMX_O_JOINT_POS: p = st->joint_pos; name = "joint_pos"; break;
            case IMX_O_JOINT_POS_REL: p = (st->joint_pos && st->default_joint_pos) ? (const void*)1 : nullptr; name = "joint_pos/default_joint_pos"; break;
            case IMX_O_JOINT_POS_LIMIT_NORMALIZED: p = (st->joint_pos && st->soft_joint_pos_limits) ? (const void*)1 : nullptr; name = "joint_pos/soft_joint_pos_limits"; break;
            case IMX_O_JOINT_VEL: p = st->joint_vel; name = "joint_vel"; break;
            case IMX_O_JOINT_VEL_REL: p = (st->joint_vel && st->default_joint_vel) ? (const void*)1 : nullptr; name = "joint_vel/default_joint_vel"; break;
            case IMX_O_LAST_ACTION: p = bf->action; name = "action"; break;
            case IMX_O_GENERATED_COMMANDS: p = st->command; name = "command"; break;
            case IMX_O_BODY_INCOMING_WRENCH: p = st->link_incoming_joint_force; name = "link_incoming_joint_force"; break;
            case IMX_O_HEIGHT_SCAN: case IMX_O_EXTERNAL: case IMX_O_OBJECT_POSITION_IN_ROBOT_ROOT_FRAME: case IMX_O_GOAL_QUAT_DIFF:
                IMX_FAIL("imx_pretrained_policy: observation record %d (op %d) is not built into the fused low-level step", k, op);
            default: break;
        }
        IMX_REQUIRE(p, "imx_pretrained_policy: state tensor '%s' is required by an observation term but missing", name);
    }
    for (int k = 0; k < plan->nact; ++k)
        IMX_REQUIRE(w[plan->act_off + k * IMX_REC_WORDS + IMX_R_OP] == IMX_A_JOINT_AFFINE, "imx_pretrained_policy: action record %d is no joint action", k);
    if (imx_check_action_inputs(plan, st, bf, "imx_pretrained_policy")) return 1;
    return 0;
}

// (the argument checks alone, for the CPU suite: 0 = the launch would be made)
extern "C" int imx_pretrained_policy_check(const imx_plan_t* ll_plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                                           const imx_pretrained_policy_t* policy, int tile_rows) {
    return pp_check(ll_plan, N, st, bf, policy, tile_rows);
}

extern "C" int imx_pretrained_policy(const imx_plan_t* plan, int64_t N, const imx_state_t* st, const imx_buffers_t* bf,
                                     const imx_pretrained_policy_t* pol, const float* noise_u_d, uint64_t seed, const int32_t* step_counter_d,
                                     int32_t step_stride, int32_t step_offset, int enable_corruption, int tile_rows, float* obs_out_d,
                                     imx_stream_t stream) {
    if (pp_check(plan, N, st, bf, pol, tile_rows)) return 1;
    IMX_REQUIRE(plan->dev, "imx_pretrained_policy: plan has no device copy (no GPU visible when it was created)");
    const int rows = tile_rows ? tile_rows : imx_pretrained_policy_tile_rows(N);
    const bool packed = rows == 32 && pol->packed_weights_d[0] != nullptr;
    PolicyArgs a{};
    a.N = N;
    a.nlayers = pol->nlayers;
    for (int l = 0; l < pol->nlayers; ++l) {
        a.W[l] = packed ? pol->packed_weights_d[l] : pol->weights_d[l];
        a.b[l] = pol->biases_d[l];
        a.ldw[l] = pol->weight_pitch[l];
    }
    for (int l = 0; l <= pol->nlayers; ++l) a.dim[l] = pol->dims[l];
    a.alpha = pol->elu_alpha;
    a.noise_u = noise_u_d; a.seed = seed; a.step_d = step_counter_d; a.step_stride = step_stride; a.step_offset = step_offset;
    a.corrupt = enable_corruption & 1;
    a.obs_out = obs_out_d;
    const size_t lds = (2ull * rows * INF_PITCH + (size_t)rows * IMX_PP_ES) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        const size_t lds32 = (2ull * 32 * INF_PITCH + 32ull * IMX_PP_ES) * sizeof(float), lds16 = (2ull * 16 * INF_PITCH + 16ull * IMX_PP_ES) * sizeof(float);
        IMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pretrained_policy<16, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds16));
        IMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pretrained_policy<32, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
        IMX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pretrained_policy<32, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
        attr_set = true;
    }
    const PlanView pv = imx_plan_view(plan);
    const dim3 grid((unsigned)((N + rows - 1) / rows)), bs(256);
    hipStream_t s = (hipStream_t)stream;
    if (rows == 16) hipLaunchKernelGGL((k_pretrained_policy<16, false>), grid, bs, lds, s, pv, *st, *bf, a);
    else if (packed) hipLaunchKernelGGL((k_pretrained_policy<32, true>), grid, bs, lds, s, pv, *st, *bf, a);
    else hipLaunchKernelGGL((k_pretrained_policy<32, false>), grid, bs, lds, s, pv, *st, *bf, a);
    IMX_HIP(hipGetLastError());
    return 0;
}
