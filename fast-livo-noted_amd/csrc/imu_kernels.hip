// imu_kernels.hip — CDNA4 (gfx950) kernel of the IMU forward propagation:
// ImuProcess::UndistortPcl, IMU_Processing.cpp:236-338 (the loop over IMU
// samples, the frame-end prediction and the carry between calls).
//
//   k_imu_propagate   one wave64 per job (grid = jobs).  The trajectory (R, v,
//       p, the Pose6D rows, the end pose) is wave-uniform: every lane computes
//       it in doubles in the reference's expression order, lane 0 stores it.
//       The covariance stays in LDS for the whole job.  F_x is the identity
//       plus six 3 x 3 blocks,
//             rows 0-2:  Exp(w, -dt) at cols 0-2,  -dt I at cols 9-11
//             rows 3-5:  dt I at cols 6-8
//             rows 6-8:  -R [a]x dt at cols 0-2,  -R dt at cols 12-14,  dt I at cols 15-17
//       so F_x P F_x^T changes rows and columns 0-8 only: a row pass (lane c
//       owns column c: 18 old entries into registers, 9 new ones back) and,
//       behind a barrier, the same map as a column pass (lane r owns row r),
//       which also adds cov_w's four diagonal blocks.  No dense 18^3 product,
//       no global traffic for P between samples.  The samples come through
//       LDS in chunks of 64 (one coalesced read a chunk); each propagated
//       sample writes its 22-double Pose6D row.
//
// Numerics: -ffp-contract=off.  The sums of the covariance passes run left to
// right over the blocks above (Eigen's GEMM order is its own).
#include <hip/hip_runtime.h>
#include <math.h>

#include "livo_internal.h"
#include "so3_device.h"

namespace livo {

constexpr int kImuN = LIVO_DIM_STATE;
constexpr int kImuRow = 22;      // Pose6D: offset_time, acc, gyr, vel, pos, rot
constexpr int kImuChunk = 64;    // samples staged in LDS at a time
constexpr int kImuSampleD = 7;   // stamp, acc, gyr
static_assert(sizeof(livo_imu_sample) == kImuSampleD * sizeof(double), "livo_imu_sample is 7 doubles");
static_assert(sizeof(livo_imu_pose) == kImuRow * sizeof(double), "Pose6D row");

// o[0..8] = rows 0-8 of F_x x for a column x of P (or, for a row x of F_x P, columns 0-8 of x F_x^T)
__device__ __forceinline__ void imu_fx_apply(const double* x, const double* A, const double* Bm, const double* Cm,
                                             double dt, double* o) {
    const double ndt = -dt;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        o[i] = ((A[i * 3 + 0] * x[0] + A[i * 3 + 1] * x[1]) + A[i * 3 + 2] * x[2]) + ndt * x[9 + i];
        o[3 + i] = x[3 + i] + dt * x[6 + i];
        o[6 + i] = ((((Bm[i * 3 + 0] * x[0] + Bm[i * 3 + 1] * x[1]) + Bm[i * 3 + 2] * x[2]) + x[6 + i]) +
                    ((Cm[i * 3 + 0] * x[12] + Cm[i * 3 + 1] * x[13]) + Cm[i * 3 + 2] * x[14])) +
                   dt * x[15 + i];
    }
}

__device__ __forceinline__ void imu_store_row(double* row, double t, const double* acc, const double* gyr,
                                              const double* vel, const double* pos, const double* R) {
    row[0] = t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        row[1 + k] = acc[k];
        row[4 + k] = gyr[k];
        row[7 + k] = vel[k];
        row[10 + k] = pos[k];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) row[13 + k] = R[k];
}

__global__ __launch_bounds__(64) void k_imu_propagate(ImuBatch B) {
    __shared__ double P[kImuN * kImuN];
    __shared__ double S[kImuChunk * kImuSampleD];
    const int j = blockIdx.x, lane = threadIdx.x;
    const ImuJobDev J = B.jobs[j];
    livo_state* st = B.states + j;
    livo_imu_carry* cy = B.carries + j;
    for (int i = lane; i < kImuN * kImuN; i += 64) P[i] = st->cov[i];

    double R[9], vel[3], pos[3], bg[3], ba[3], grav[3], acc_imu[3], angvel[3], head[kImuSampleD];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = st->rot[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        vel[k] = st->vel[k];
        pos[k] = st->pos[k];
        bg[k] = st->bias_g[k];
        ba[k] = st->bias_a[k];
        grav[k] = st->gravity[k];
        acc_imu[k] = cy->acc_s_last[k];
        angvel[k] = cy->angvel_last[k];
        head[1 + k] = cy->last_imu.acc[k];
        head[4 + k] = cy->last_imu.gyr[k];
    }
    head[0] = cy->last_imu.stamp;
    const double last_end = cy->last_lidar_end_time;
    double* rows = B.poses ? B.poses + (int64_t)j * B.pose_cap * kImuRow : nullptr;
    // IMUpose[0] (:238)
    if (rows && lane == 0 && B.pose_cap > 0) imu_store_row(rows, 0.0, acc_imu, angvel, vel, pos, R);
    int np = 1;

    for (int base = 0; base < J.n_imu; base += kImuChunk) {
        __syncthreads();  // the previous chunk has been read (and P's load is done)
        if (base + lane < J.n_imu) {
            const double* s = reinterpret_cast<const double*>(B.samples + J.first + base + lane);
#pragma unroll
            for (int k = 0; k < kImuSampleD; k++) S[lane * kImuSampleD + k] = s[k];
        }
        __syncthreads();
        const int m = min(kImuChunk, J.n_imu - base);
        for (int t = 0; t < m; t++) {
            double tail[kImuSampleD];
#pragma unroll
            for (int k = 0; k < kImuSampleD; k++) tail[k] = S[t * kImuSampleD + k];
            if (!(tail[0] < last_end)) {  // (:251; wave-uniform)
                double acc[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    angvel[k] = 0.5 * (head[4 + k] + tail[4 + k]) - bg[k];
                    acc[k] = ((0.5 * (head[1 + k] + tail[1 + k])) * 9.81) / B.acc_norm - ba[k];
                }
                const double dt = head[0] < last_end ? tail[0] - last_end : tail[0] - head[0];
                double Ef[9], A[9], Bm[9], Cm[9], Qa[9];
                so3_exp_dt(angvel, dt, Ef);
                so3_exp_dt(angvel, -dt, A);
                const double sk[9] = {0.0, -acc[2], acc[1], acc[2], 0.0, -acc[0], -acc[1], acc[0], 0.0};
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        Bm[i * 3 + c] = (((-R[i * 3 + 0]) * sk[0 * 3 + c] + (-R[i * 3 + 1]) * sk[1 * 3 + c]) +
                                         (-R[i * 3 + 2]) * sk[2 * 3 + c]) * dt;
                        Cm[i * 3 + c] = (-R[i * 3 + c]) * dt;
                        Qa[i * 3 + c] = ((((R[i * 3 + 0] * B.cov_acc[0]) * R[c * 3 + 0] +
                                           (R[i * 3 + 1] * B.cov_acc[1]) * R[c * 3 + 1]) +
                                          (R[i * 3 + 2] * B.cov_acc[2]) * R[c * 3 + 2]) * dt) * dt;
                    }
                // row pass: F_x P (lane c: column c)
                if (lane < kImuN) {
                    double x[kImuN], o[9];
#pragma unroll
                    for (int k = 0; k < kImuN; k++) x[k] = P[k * kImuN + lane];
                    imu_fx_apply(x, A, Bm, Cm, dt, o);
#pragma unroll
                    for (int k = 0; k < 9; k++) P[k * kImuN + lane] = o[k];
                }
                __syncthreads();
                // column pass: (F_x P) F_x^T + cov_w (lane r: row r)
                if (lane < kImuN) {
                    double x[kImuN], o[9];
#pragma unroll
                    for (int k = 0; k < kImuN; k++) x[k] = P[lane * kImuN + k];
                    imu_fx_apply(x, A, Bm, Cm, dt, o);
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        if (lane == i) o[i] = o[i] + (B.cov_gyr[i] * dt) * dt;
                        if (lane == 6 + i) {
#pragma unroll
                            for (int c = 0; c < 3; c++) o[6 + c] = o[6 + c] + Qa[i * 3 + c];
                        }
                        // rows 9-14: cov_w lies on their diagonal, beyond the columns this pass rewrites
                        if (lane == 9 + i) P[lane * (kImuN + 1)] = x[9 + i] + (B.cov_bias_gyr[i] * dt) * dt;
                        if (lane == 12 + i) P[lane * (kImuN + 1)] = x[12 + i] + (B.cov_bias_acc[i] * dt) * dt;
                    }
#pragma unroll
                    for (int k = 0; k < 9; k++) P[lane * kImuN + k] = o[k];
                }
                __syncthreads();
                // attitude, specific force in the world frame, position, velocity (:301-310)
                double Rn[9];
                m3m(R, Ef, Rn);
#pragma unroll
                for (int k = 0; k < 9; k++) R[k] = Rn[k];
                m3v(R, acc, acc_imu);
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    acc_imu[k] = acc_imu[k] + grav[k];
                    pos[k] = (pos[k] + vel[k] * dt) + ((0.5 * acc_imu[k]) * dt) * dt;
                    vel[k] = vel[k] + acc_imu[k] * dt;
                }
                if (rows && lane == 0 && np < B.pose_cap)
                    imu_store_row(rows + (int64_t)np * kImuRow, tail[0] - J.pcl_beg, acc_imu, angvel, vel, pos, R);
                np++;
            }
#pragma unroll
            for (int k = 0; k < kImuSampleD; k++) head[k] = tail[k];
        }
    }
    __syncthreads();

    // the prediction at the frame end (:320-335); head = v_imu.back()
    const double imu_end = head[0];
    const double from = imu_end > J.pcl_beg ? imu_end : J.pcl_beg;
    const double note = J.pcl_end > from ? 1.0 : -1.0;
    const double dt = note * (J.pcl_end - from);
    double nw[3], Ee[9], Re[9];
#pragma unroll
    for (int k = 0; k < 3; k++) nw[k] = note * angvel[k];
    so3_exp_dt(nw, dt, Ee);
    m3m(R, Ee, Re);
    for (int i = lane; i < kImuN * kImuN; i += 64) st->cov[i] = P[i];
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) st->rot[k] = Re[k];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            st->vel[k] = vel[k] + (note * acc_imu[k]) * dt;
            st->pos[k] = (pos[k] + (note * vel[k]) * dt) + (((note * 0.5) * acc_imu[k]) * dt) * dt;
            cy->acc_s_last[k] = acc_imu[k];
            cy->angvel_last[k] = angvel[k];
            cy->last_imu.acc[k] = head[1 + k];
            cy->last_imu.gyr[k] = head[4 + k];
        }
        cy->last_imu.stamp = head[0];
        cy->last_lidar_end_time = J.pcl_end;
        B.n_poses[j] = np;
    }
}

int launch_imu_propagate(const ImuBatch& B, int32_t n, void* stream) {
    if (n <= 0) return LIVO_OK;
    hipLaunchKernelGGL(k_imu_propagate, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, B);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
