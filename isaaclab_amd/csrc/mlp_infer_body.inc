// The body of k_mlp_infer / k_mlp_infer_binary (mlp.hip), included once per kernel with IMX_ACT_BINARY = false (the kernel as it always was) or true (the actor
// head's epilogue with the binary joint term's path).  A textual include, not a device function: the existing kernels then compile to the
// instruction streams they had.  Also the body of k_mlp_infer2 / k_mlp_infer2_binary (IMX_INFER_TWO_INPUTS = 1, below) and of
// k_mlp_infer2n / k_mlp_infer2n_binary (IMX_INFER_NORMALIZE = 1 on top of it: the rows are normalised between load and LDS store).
    extern __shared__ float smem[];  // two activation buffers of INF_ROWS x INF_PITCH floats
    float* buf0 = smem;
    float* buf1 = smem + INF_ROWS * INF_PITCH;
    const int which = blockIdx.x / a.tiles;
    const InferNet& net = a.net[which];
    const int64_t m0 = (int64_t)(blockIdx.x - which * a.tiles) * INF_ROWS;
    const bool act_here = act.enabled && which == 0;  // the actor's workgroups finish PPO.act + ActionManager.process_action themselves
    // Where the input rows come from, and whether the tile is also stored densely on its way into LDS.  IMX_INFER_TWO_INPUTS = 0 are macros
    // that spell what the body always said (same tokens, same kernels); 1 (k_mlp_infer2*, argument `two`): network 1 reads its own
    // input and may keep its rows as well (storage.privileged_observations[t])
#if IMX_INFER_TWO_INPUTS
    const float* const x_in = which ? two.X1 : a.X;
    const int64_t ldx_in = which ? two.ldx1 : a.ldx;
    float* const obs_dst = which ? two.obs_out1 : (act.enabled ? act.obs_out : nullptr);
#define IMX_INFER_X x_in
#define IMX_INFER_LDX ldx_in
#define IMX_INFER_OBS_ON (obs_dst != nullptr)
#define IMX_INFER_OBS_DST obs_dst
#else
#define IMX_INFER_X a.X
#define IMX_INFER_LDX a.ldx
#define IMX_INFER_OBS_ON act_here
#define IMX_INFER_OBS_DST act.obs_out
#endif
    // input rows -> LDS (the 32 rows are one contiguous run when ldx == dim[0]); columns up to the next multiple of 32 are zeroed
    const int K0 = net.dim[0], K0p = (K0 + 31) & ~31;
    {
        // wave w takes rows w, w+4, ...; lanes run along the row.  ALL loads of the tile are issued before the first LDS store -- one HBM
        // round trip for the whole input (a load -> store loop pays one per iteration: 16 us for 235 columns; two half tiles paid two) --
        // and only the 64-column pieces the input has (a clamped load of a piece past K0 is still a memory request).
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const int ncc = (K0 + 63) >> 6;  // (uniform)
        float v[8][INF_MAXD / 64];
#if IMX_INFER_NORMALIZE
        // (k_mlp_infer2n*, argument `nrm`) the lane's mean / std of its columns ride in the tile's load batch; a null pair (uniform): rows as they are
        const float* const n_mean = nrm.mean[which];
        const float* const n_std = nrm.stdv[which];
        float nmu[INF_MAXD / 64], nsd[INF_MAXD / 64];
#pragma unroll
        for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
            const int c = lane + 64 * cc;
            nmu[cc] = (n_mean && cc < ncc) ? n_mean[c < K0 ? c : 0] : 0.0f;
            nsd[cc] = (n_mean && cc < ncc) ? n_std[c < K0 ? c : 0] : 1.0f;
        }
#endif
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int row = w + 4 * rr;
            const float* src = IMX_INFER_X + (m0 + row < a.M ? m0 + row : 0) * IMX_INFER_LDX;
#pragma unroll
            for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                if (cc < ncc) {
                    const int c = lane + 64 * cc;
                    const float x = src[c < K0 ? c : 0];  // clamped, unconditional within the piece
                    v[rr][cc] = (c < K0 && m0 + row < a.M) ? x : 0.0f;
                } else {
                    v[rr][cc] = 0.0f;
                }
            }
        }
#if IMX_INFER_NORMALIZE
        if (n_mean) {  // k_norm_apply's expression (a true division): LDS and the dense store get what an apply launch would have left
            const float n_eps = nrm.eps[which];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int row = w + 4 * rr;
#pragma unroll
                for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                    const int c = lane + 64 * cc;
                    if (c < K0 && m0 + row < a.M) v[rr][cc] = (v[rr][cc] - nmu[cc]) / (nsd[cc] + n_eps);  // (padding and rows past M stay zero)
                }
            }
        }
#endif
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int row = w + 4 * rr;
#pragma unroll
            for (int cc = 0; cc < INF_MAXD / 64; ++cc) {
                const int c = lane + 64 * cc;
                if (c < K0p) buf0[row * INF_PITCH + c] = v[rr][cc];
                if (IMX_INFER_OBS_ON && c < K0 && m0 + row < a.M) IMX_INFER_OBS_DST[(m0 + row) * (int64_t)K0 + c] = v[rr][cc];  // storage.observations[t]
            }
        }
    }
    __syncthreads();
    float* in = buf0;
    float* out = buf1;
    for (int l = 0; l < net.nlayers; ++l) {
        const int K = net.dim[l], N = net.dim[l + 1];
        const bool last = l == net.nlayers - 1;
        const int nbw = ((N + 31) / 32 + 3) / 4;  // 32-column blocks per wave
        float* so = (last && !act_here) ? nullptr : out;  // (the actor head of imx_mlp_infer_act keeps its means in LDS)
        if (!last) {  // zero the padding columns the next layer's 32-wide reduction groups will read
            const int Np = (N + 31) & ~31;
            for (int i = threadIdx.x; i < INF_ROWS * (Np - N); i += blockDim.x) {
                const int row = i / (Np - N), col = N + i - row * (Np - N);
                out[row * INF_PITCH + col] = 0.0f;
            }
        }
        const float* Wl = PACKED ? net.Wp[l] : net.W[l];
        if (nbw <= 1) infer_layer<1, PACKED>(in, K, Wl, net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        else if (nbw == 2) infer_layer<2, PACKED>(in, K, Wl, net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        else infer_layer<4, PACKED>(in, K, Wl, net.ldw[l], net.b[l], N, !last, net.alpha, so, net.out, m0, a.M);
        __syncthreads();
        float* t = in; in = out; out = t;
    }
    if (act_here) act_epilogue<INF_ROWS, IMX_ACT_BINARY>(act, in, out, m0, a.M);
#undef IMX_INFER_X
#undef IMX_INFER_LDX
#undef IMX_INFER_OBS_ON
#undef IMX_INFER_OBS_DST
