// lio_kernels.hip — CDNA4 (gfx950) kernel of livo_lio_frame: the IEKF slot staged on the device.
//
//   k_lio_stage_slot   one wave64.  Reads the propagated livo_state where k_imu_propagate left it
//       and writes the complete LaserMapping slot that init_slot + cov_factor (livo_capi.cpp) would
//       have uploaded: state = prior = the propagated state, the control block, covL / covB /
//       cov_ok, zeros elsewhere (the reduction's tickets included).  Every 8-byte word of the slot
//       is stored exactly once, so no store order inside the wave matters.
//
//       The covariance comes through LDS once (coalesced).  The tests over rows and columns 0-5
//       of P take one entry per lane.  The 6 x 6 Cholesky is wave-uniform: every lane runs
//       cov_factor's loops in its order from LDS (a serial chain of 6 square roots and 15
//       divisions, not spread over lanes).  Row r of
//       B depends only on L and row r of P: lane r - 6 owns it (12 lanes).  A rejection does not
//       leave early, it clears `ok` and the arithmetic runs on (its results are not stored), so
//       cov_ok is 0 on exactly the inputs where the host returns before setting it.
//
// Numerics: doubles, -ffp-contract=off, IEEE division and square root: the host's bits.
// Visibility: plain stores.  The evaluation kernels read the slot in later launches on the same
// stream (their sc1 loads bypass the L1, which holds nothing of the slot at their start).
#include <hip/hip_runtime.h>
#include <math.h>

#include "livo_internal.h"

namespace livo {

constexpr int kLioD = LIVO_DIM_STATE;
constexpr int kLioStateWords = (int)(sizeof(livo_state) / 8);
constexpr int kLioSlotWords = (int)(kSlotLmBytes / 8);
constexpr int kLioCtrlWord = (int)(offsetof(IekfSlot, ctrl) / 8);
constexpr int kLioCtrlWords = (int)(sizeof(IekfCtrl) / 8);
constexpr int kLioCovWord = (int)(offsetof(IekfSlot, covL) / 8);
constexpr int kLioCovWords = 36 + (kLioD - 6) * 6 + 1;  // covL, covB and the word of cov_ok
static_assert(sizeof(livo_state) % 8 == 0 && kSlotLmBytes % 8 == 0, "the slot is staged in 8-byte words");
static_assert(offsetof(IekfSlot, state) == 0 && offsetof(IekfSlot, prior) == sizeof(livo_state), "state, prior lead");
static_assert(offsetof(IekfSlot, ctrl) % 8 == 0 && sizeof(IekfCtrl) == 32, "control block: four words");
static_assert(offsetof(IekfSlot, covL) % 8 == 0 && offsetof(IekfSlot, covB) == offsetof(IekfSlot, covL) + 36 * 8 &&
                  offsetof(IekfSlot, cov_ok) == offsetof(IekfSlot, covB) + (kLioD - 6) * 6 * 8,
              "covL, covB, cov_ok contiguous");
static_assert(kLioD - 6 <= 64, "one lane per row of B");

__global__ __launch_bounds__(64) void k_lio_stage_slot(const livo_state* __restrict__ src, IekfSlot* __restrict__ slot,
                                                       int max_iter) {
    __shared__ double P[kLioD * kLioD];
    __shared__ double Ls[36];
    const int lane = threadIdx.x;
    for (int i = lane; i < kLioD * kLioD; i += 64) P[i] = src->cov[i];
    // state, prior and the zeros: every word outside the control block and the factors
    {
        const unsigned long long* s = reinterpret_cast<const unsigned long long*>(src);
        unsigned long long* d = reinterpret_cast<unsigned long long*>(slot);
        for (int w = lane; w < kLioSlotWords; w += 64) {
            if (w >= kLioCtrlWord && w < kLioCtrlWord + kLioCtrlWords) continue;
            if (w >= kLioCovWord && w < kLioCovWord + kLioCovWords) continue;
            d[w] = w < 2 * kLioStateWords ? s[w < kLioStateWords ? w : w - kLioStateWords] : 0ull;
        }
    }
    if (lane == 0) {  // init_slot's control block: the first evaluation searches, iterCount starts at -1
        IekfCtrl ct;
        ct.stop = 0;
        ct.search_en = 1;
        ct.iter_count = -1;
        ct.rematch_num = 0;
        ct.converged = 0;
        ct.n_evals = 0;
        ct.max_iter = max_iter;
        ct.last_search = 0;
        slot->ctrl = ct;
    }
    __syncthreads();
    constexpr int D = kLioD;
    bool ok = true;
    // cov_factor's two passes over rows and columns 0-5: lane e and e + 64 take entry (i, j) = (e / 6,
    // e % 6) of the 18 x 6.  amax is a maximum of finite values (any other input is rejected), so the
    // order it is taken in does not change its bits.
    double amax = 0.0;
    bool bad = false;
#pragma unroll 1
    for (int e = lane; e < D * 6; e += 64) {
        const int i = e / 6, j = e - 6 * i;
        const double a = P[i * D + j], b = P[j * D + i];
        if (!isfinite(a) || !isfinite(b)) bad = true;
        const double fa = fabs(a);
        amax = amax < fa ? fa : amax;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(amax, off, 64);
        amax = amax < o ? o : amax;
    }
#pragma unroll 1
    for (int e = lane; e < D * 6; e += 64) {
        const int i = e / 6, j = e - 6 * i;
        if (fabs(P[i * D + j] - P[j * D + i]) > 1e-12 * amax) bad = true;
    }
    if (__any(bad)) ok = false;
    // S = L L^T in cov_factor's loop order (wave-uniform, registers: every index is static)
    double Lm[36];
#pragma unroll
    for (int k = 0; k < 36; k++) Lm[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = P[j * D + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= Lm[j * 6 + k] * Lm[j * 6 + k];
        if (!(d > 1e-13 * P[j * D + j]) || !(d > 0.0)) ok = false;  // not (numerically) positive definite
        const double l = sqrt(d);
        Lm[j * 6 + j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = P[i * D + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= Lm[i * 6 + k] * Lm[j * 6 + k];
            Lm[i * 6 + j] = v / l;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 36; k++) Ls[k] = Lm[k];
    }
    // B(r, :) L^T = P(r, 0:6): forward substitution, lane r - 6 owns row r
    double Br[6];
    bool fin = true;
    {
        const int r = 6 + (lane < D - 6 ? lane : 0);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double v = P[r * D + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= Br[k] * Lm[j * 6 + k];
            Br[j] = v / Lm[j * 6 + j];
            if (!isfinite(Br[j])) fin = false;
        }
    }
    if (__any(lane < D - 6 && !fin)) ok = false;
    __syncthreads();
    if (lane < 36) slot->covL[lane] = ok ? Ls[lane] : 0.0;
    if (lane < D - 6) {
#pragma unroll
        for (int j = 0; j < 6; j++) slot->covB[lane * 6 + j] = ok ? Br[j] : 0.0;
    }
    if (lane == 0) {
        slot->cov_ok = ok ? 1 : 0;
        slot->pad2_[0] = 0;
    }
}

int launch_lio_stage_slot(const livo_state* src, IekfSlot* slot, int max_iter, void* stream) {
    if (!src || !slot) return LIVO_E_INVALID;
    hipLaunchKernelGGL(k_lio_stage_slot, dim3(1), dim3(64), 0, (hipStream_t)stream, src, slot, max_iter);
    return hipGetLastError() == hipSuccess ? LIVO_OK : LIVO_E_HIP;
}

}  // namespace livo
