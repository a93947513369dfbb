#ifndef IMX_NORMALIZATION_STRUCT_H_
#define IMX_NORMALIZATION_STRUCT_H_
/* The structs of EmpiricalNormalization inside the fused rollout: imx_norm_group_t (one normaliser's batch for
 * imx_empirical_normalization_update) and imx_infer_norm_t (one network's statistics for imx_mlp_infer_act2n).  A header of its own,
 * included by imx.h, like imx_pose2d_struct.h; it can be included alone. */
#include <stdint.h>

typedef struct imx_norm_group {
    int64_t N;          /* rows of the batch */
    int64_t D;          /* columns */
    const float* x_d;   /* (N, D) rows with pitch ldx >= D floats */
    int64_t ldx;
    float* mean_d;      /* (D) running statistics, updated in place */
    float* var_d;
    float* std_d;
    int64_t* count_d;   /* (1) upstream's long buffer */
    int64_t until;      /* stop updating once count >= until; < 0: never stop */
    float* partials_d;  /* imx_empirical_normalization_partials_bytes(N, D) bytes of scratch, this group's own */
} imx_norm_group_t;

typedef struct imx_infer_norm {
    const float* mean_d; /* (input width of the network) */
    const float* std_d;  /* (input width of the network) */
    float eps;
} imx_infer_norm_t;

#endif
