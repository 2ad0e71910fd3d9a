// lattice.h -- what the one-wave-per-utterance lattice kernels share (ctc_align.hip, asg.hip, asg_align.hip): the clamps of
// lengths and labels, the neighbour-lane move, and the windows of backpointer rows that a backtrace pulls from HBM into LDS.
#pragma once
#include "common.h"

__device__ __forceinline__ int clamp_label(int c, int k) { return c < 0 ? 0 : (c >= k ? k - 1 : c); }

__device__ __forceinline__ void clamp_lengths(const int32_t* label_len, const int32_t* input_len, int b, int l_max, int t_out,
                                              int& L, int& T) {
    L = label_len[b];
    L = L < 0 ? 0 : (L > l_max ? l_max : L);
    T = input_len[b];
    T = T < 0 ? 0 : (T > t_out ? t_out : T);
}

__device__ __forceinline__ float dpp_float_from_lower_lane(float v, float lane0_value) {  // lane l <- lane l-1
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0_value), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

constexpr int BT_W = 64;  // frames per backtrace window (one per lane)

// backtrace window w of an utterance's HBM rows of R bytes (rows w*BT_W .. min(T, w*BT_W + BT_W) - 1: one contiguous range)
// into V registers of type Vec per lane (V * 64 * sizeof(Vec) == BT_W * R), and from there into LDS window buffer w & 1
template <typename Vec, int V, int R>
__device__ __forceinline__ void load_window(Vec (&wreg)[V], const uint8_t* bp_utt, int w, int T, int lane) {
    const int w0 = w * BT_W;
    const int n = ((T - w0 < BT_W ? T - w0 : BT_W) * R) / (int)sizeof(Vec);
    const Vec* src = (const Vec*)(bp_utt + (long)w0 * R);
#pragma unroll
    for (int m = 0; m < V; ++m) {
        const int i = m * 64 + lane;
        if (i < n) wreg[m] = src[i];
    }
}
template <typename Vec, int V, int R>
__device__ __forceinline__ void store_window(const Vec (&wreg)[V], uint8_t* rows, int w, int lane) {
    Vec* dst = (Vec*)(rows + (w & 1) * BT_W * R);
#pragma unroll
    for (int m = 0; m < V; ++m) dst[m * 64 + lane] = wreg[m];
}
