// ctc_shared.h -- what ctc.hip (the wave lattice: labels of up to 255 letters, k <= 63; the fp32 log-domain lattice of
// sl_ctc_select(1) up to 511) and ctc_long.hip (everything else up to 2047 letters) both need: the lattice units, the wave
// reductions, the row stride of a lattice and the entry point of the double log-domain path.  Kernels stay in their own files.
#pragma once
#include "common.h"

// longest label of sl_ctc_loss_grad: 4095 lattice states (include/speechless_hip.h says why not the aligners' 8191)
constexpr int SL_CTC_MAX_LABEL = 2047;
// longest label of any kernel of ctc.hip (ctc_lattice_kernel, one lattice state per thread: 2 * 511 + 1 <= 1024); beyond it
// ctc_long.hip whatever sl_ctc_select says
constexpr int SL_CTC_SHORT_MAX_LABEL = 511;

namespace {

// The lattices live in LOG2 units: v_exp_f32 / v_log_f32 are base-2 natively.
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// row stride of a log-domain lattice: the 2 * l_max + 1 states rounded up to whole waves of columns
__host__ int lattice_sp(int l_max) { return ((2 * l_max + 1) + 63) / 64 * 64; }

}  // namespace

// ctc_long.hip: sl_ctc_loss_grad for 1 <= l_max <= 2047, 2 <= k <= 64 (arguments validated and the workspace laid out by ctc.hip,
// which sends it every call the wave lattice does not take: 2 * l_max + 1 > 512 or k > 63).
// alpha, beta: [batch][t_out][lattice_sp(l_max)] doubles; cls: [batch][l_max + k + 1]; logz2, zint: [batch];
// dump: ctc_long_dump_bytes(batch) bytes (where the lanes beyond a row's end put their stores).
size_t ctc_long_dump_bytes(int batch);
int ctc_long_loss_grad(const float* probs, const float* logq, const int32_t* labels, const int32_t* label_len,
                       const int32_t* input_len, float* loss, void* dlogits, int batch, int t_out, int k, int l_max, int g_row0,
                       int g_row_stride, long g_batch_stride, int out_f32, float eps, float grad_scale, double* alpha,
                       double* beta, int32_t* cls, float* logz2, int32_t* zint, double* dump, hipStream_t s);
