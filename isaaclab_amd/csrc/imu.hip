// Imu sensor (isaaclab/sensors/imu/imu.py under SensorBase): imx_imu, one launch for up to IMX_MAX_IMU sensors, and imx_plan_bind_imu,
// which hands a plan the data tensors its imu_* observation terms read.
#include "imx_internal.h"
#include "imx_imu.h"

struct ImuSensors {
    imx_imu_t s[IMX_MAX_IMU];
};

// Lane = (sensor, env): blockIdx.y is the sensor, so its struct is a wave-uniform read of the kernel arguments.  A few hundred bytes
// per env and no reuse: latency-bound, nothing to tune.
__global__ void __launch_bounds__(256) k_imu(ImuSensors S, int64_t N) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    imu_env(S.s[blockIdx.y], e);
}

extern "C" int imx_imu(const imx_imu_t* sensors, int32_t num_sensors, int64_t N, imx_stream_t stream) {
    IMX_REQUIRE(sensors, "imx_imu: null argument");
    IMX_REQUIRE(num_sensors >= 1 && num_sensors <= IMX_MAX_IMU, "imx_imu: %d sensors in one launch (1..%d)", (int)num_sensors, IMX_MAX_IMU);
    IMX_REQUIRE(N > 0 && N < (1ll << 31), "imx_imu: N out of range");
    ImuSensors S{};
    for (int k = 0; k < num_sensors; ++k) {
        if (const char* why = imu_check(&sensors[k])) IMX_FAIL("imx_imu: sensor %d: %s", k, why);
        S.s[k] = sensors[k];
    }
    hipLaunchKernelGGL(k_imu, dim3((unsigned)((N + 255) / 256), (unsigned)num_sensors), dim3(256), 0, (hipStream_t)stream, S, N);
    IMX_HIP(hipGetLastError());
    return 0;
}

extern "C" int imx_plan_bind_imu(imx_plan_t* plan, const imx_imu_t* sensors, int32_t num_sensors) {
    IMX_REQUIRE(plan, "imx_plan_bind_imu: null plan");
    IMX_REQUIRE(num_sensors >= 0 && num_sensors <= IMX_MAX_IMU && (sensors || num_sensors == 0), "imx_plan_bind_imu: %d sensors (0..%d)",
                (int)num_sensors, IMX_MAX_IMU);
    plan->imu = ImuObsView{};
    for (int k = 0; k < num_sensors; ++k) {
        IMX_REQUIRE(sensors[k].quat_w_d && sensors[k].ang_vel_b_d && sensors[k].lin_acc_b_d, "imx_plan_bind_imu: sensor %d: a data tensor is missing", k);
        plan->imu.quat_w[k] = sensors[k].quat_w_d;
        plan->imu.ang_vel_b[k] = sensors[k].ang_vel_b_d;
        plan->imu.lin_acc_b[k] = sensors[k].lin_acc_b_d;
    }
    plan->n_imu = num_sensors;
    return 0;
}
