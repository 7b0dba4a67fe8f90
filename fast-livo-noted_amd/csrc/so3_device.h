// so3_device.h — SO(3) helpers shared by the device kernels that restate the
// reference's IMU arithmetic (frontend_kernels.hip: the backward walk;
// imu_kernels.hip: the forward propagation).  Doubles in the reference's
// expression order; build with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace livo {

// Exp(ang_vel, dt) (so3_math.h:31-52)
__device__ __forceinline__ void so3_exp_dt(const double* g, double dt, double* R) {
    const double nrm = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (nrm > 0.0000001) {
        const double r[3] = {g[0] / nrm, g[1] / nrm, g[2] / nrm};
        const double K[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
        const double ang = nrm * dt;
        const double s = sin(ang), c1 = 1.0 - cos(ang);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double kk = ((c1 * K[i * 3 + 0]) * K[0 * 3 + j] + (c1 * K[i * 3 + 1]) * K[1 * 3 + j]) +
                                  (c1 * K[i * 3 + 2]) * K[2 * 3 + j];
                R[i * 3 + j] = (R[i * 3 + j] + s * K[i * 3 + j]) + kk;
            }
    }
}

__device__ __forceinline__ void m3v(const double* M, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (M[i * 3 + 0] * v[0] + M[i * 3 + 1] * v[1]) + M[i * 3 + 2] * v[2];
}

// C = A B, 3 x 3 row-major
__device__ __forceinline__ void m3m(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) + A[i * 3 + 2] * B[2 * 3 + j];
}

}  // namespace livo
