// asg_align_long.hip -- ASG forced alignment of LONG recordings: sl_asg_align (asg_align.hip) beyond 511 graphemes, for gfx950.
//
// The segmentation the auto segmentation criterion is named for, for the recordings that need it most: a recording of a few
// minutes has thousands of graphemes, and alignment.cut_sections turns its alignment into training utterances.  Semantics (bit
// for bit, fp32): those of sl_asg_align, include/speechless_hip.h.  Only the limits differ: l_max <= 8191.
//
// Kernel asg_align_long_kernel<NW>: ONE WORK-GROUP of NW waves (1 / 2 / 4 / 8 / 16 for l_max <= 512 / 1024 / 2048 / 4096 / 8191)
// per recording, NS = 8 consecutive states per lane in registers: thread i holds states 8 i .. 8 i + 7, a wave 512 states.  A
// thread gathers the column of each of its states and the two scores it ever needs, g(l_s, l_s) and g(l_{s-1}, l_s), once.  Per
// frame exactly one value crosses a thread boundary: the highest state of the thread below.  Inside a wave it moves by the DPP
// wave_shr:1 of lattice.h; across waves it goes through one LDS slot per wave, double-buffered by frame parity (lane 63 of wave w
// writes slot [t & 1][w] after frame t, lane 0 of wave w + 1 reads it in frame t + 1), which costs ONE work-group barrier per
// frame.  Every barrier is uniform: all trip counts depend on the recording only, and both infeasible-row exits are taken by the
// whole work-group (the first before any barrier, the second on a score every thread reads from the same LDS word).  Per state
// and frame: stay = d(s) + g(l_s, l_s), move = d(s-1) + g(l_{s-1}, l_s), the larger (stay on a tie) plus the emission -- three
// separately rounded adds, no multiply: asg_frame of lattice.h, the very step of asg_align.hip.  Emissions come from LDS: the
// work-group stages ALIGN_CH frames of logq rows (k <= 64 floats) once for all waves while the next ALIGN_CH frames are in flight
// in registers (EmissionStager of lattice.h, with all NW waves at work).
// Backpointers: ONE bit per state and frame.  The ballot of state j's compare over a wave IS 64-bit word 8 w + j of the frame's
// row (state s at bit (s >> 3) & 63 of word (s >> 9) * 8 + (s & 7)); a row = 64 NW bytes, lanes 0 .. 7 of each wave store the
// wave's 64 bytes in one coalesced store to the workspace in HBM.
// Backtrace: wave 0 (the other waves only keep the barriers uniform).  The path drops at most one state per frame, so a window
// of BT_W = 64 frames whose top frame is at state s touches states [s - 64, s] only, and the window below it [s - 128, s]: the
// words of at most two neighbouring waves, 32 contiguous dwords of each row (all 16 with one wave).  That band of the NEXT window
// is loaded into registers (load_band / store_band of lattice.h) before the current window is resolved out of LDS, so no step of
// the T'-long chain waits on a dependent HBM load.  Lane t - w0 keeps frame t's state: one coalesced store per window.
#include <math.h>

#include "lattice.h"

namespace {

constexpr int NS = 8;           // states per thread
constexpr int WAVE_DW = 2 * NS; // backpointer dwords of a wave per frame
constexpr int L_LIMIT = 8191;

template <int NW>
struct LongBand {
    static constexpr int DW = NW == 1 ? WAVE_DW : 2 * WAVE_DW;  // dwords of a row that two windows below a state can touch
};

// LDS: [logq chunk ALIGN_CH x 64 floats][boundary slots 2 x 16][end score][backtrace windows 2 x BT_W x band dwords]
template <int NW>
struct LongLds {
    float em[ALIGN_CH * 64];
    float edge[2][16];
    float fin;
    uint32_t win[2][BT_W * LongBand<NW>::DW];
};

// first wave of the band that holds [s - 128, s]: the wave of s and the one below it
__device__ __forceinline__ int band_wave(int s) { return (s >> 9) > 0 ? (s >> 9) - 1 : 0; }

template <int NW>
__global__ __launch_bounds__(64 * NW) void asg_align_long_kernel(const float* __restrict__ logq, const float* __restrict__ trans,
                                                                 const float* __restrict__ init,
                                                                 const int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ label_len,
                                                                 const int32_t* __restrict__ input_len, int32_t* __restrict__ path,
                                                                 float* __restrict__ score, uint32_t* __restrict__ bp_hbm,
                                                                 int t_out, int k, int l_max) {
    constexpr int NT = 64 * NW;   // threads
    constexpr int BAND = LongBand<NW>::DW;
    __shared__ LongLds<NW> lds;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    const int32_t* lab = labels + (long)b * l_max;
    int32_t* prow = path + (long)b * t_out;

    for (int t = T + tid; t < t_out; t += NT) prow[t] = -1;
    if (L == 0 || T == 0 || L > T) {  // infeasible, as sl_asg_align decides (uniform over the work-group, before any barrier)
        for (int t = tid; t < T; t += NT) prow[t] = -1;
        if (tid == 0) score[b] = -INFINITY;
        return;
    }

    // per-thread states: thread i holds states 8 i .. 8 i + 7 with their emission column, stay score and move score (lattice.h)
    int col[NS];
    float gs[NS], ga[NS], d[NS];
    asg_states_init<NS>(col, gs, ga, lab, tid * NS, L, k, trans);
    const float* lq = logq + (long)b * t_out * k;
    // frame 0: only state 0 is open (here and not in a helper: see asg_states_init)
#pragma unroll
    for (int j = 0; j < NS; ++j) d[j] = tid * NS + j == 0 ? init[col[0]] + lq[col[0]] : -INFINITY;
    if (tid < 32) lds.edge[tid >> 4][tid & 15] = -INFINITY;  // frame 0: nothing at any wave's highest state but -inf

    EmissionStager<NT> stg;
    stg.prefetch(lq, 1, T, k, wave, lane);  // chunks start at frame 1
    constexpr int row_dw = WAVE_DW * NW;
    uint32_t* bp_utt = bp_hbm + (long)b * t_out * row_dw;
    for (int t0 = 1; t0 < T; t0 += ALIGN_CH) {
        // (the barrier that ended the previous chunk's last frame: every wave is done with the old rows)
        stg.store(lds.em, wave, lane);
        __syncthreads();
        if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, wave, lane);
        const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
#pragma unroll
        for (int f = 0; f < ALIGN_CH; ++f) {
            if (f >= nf) continue;  // (uniform over the work-group; a break keeps the loop from unrolling)
            const int t = t0 + f;
            float lo = dpp_float_from_lower_lane(d[NS - 1], -INFINITY);  // state NS tid - 1
            if (NW > 1 && lane == 0 && wave > 0) lo = lds.edge[(t + 1) & 1][wave - 1];  // written after frame t - 1
            uint64_t word[NS];
            asg_frame<NS>(col, gs, ga, d, lds.em + f * 64, lo, word);
            uint64_t keep = 0;  // lane j < NS keeps word j of the wave
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (lane == j) keep = word[j];
            }
            if (NW > 1 && lane == 63) lds.edge[t & 1][wave] = d[NS - 1];
            if (lane < NS) ((uint64_t*)(bp_utt + (long)t * row_dw))[wave * NS + lane] = keep;
            __syncthreads();  // the frame's barrier: boundary slots written, and (last frame of a chunk) the rows read
        }
    }

    // end state L - 1
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        if (tid * NS + j == L - 1) lds.fin = d[j];
    }
    __threadfence();
    __syncthreads();  // also orders every wave's backpointer rows before wave 0 reads them
    const float best = lds.fin;
    if (tid == 0) score[b] = best;
    if (best == -INFINITY) {  // -inf scores closed every path (uniform: one LDS word, read behind the barrier)
        for (int t = tid; t < T; t += NT) prow[t] = -1;
        return;
    }
    int s = L - 1;

    // backtrace, windows [w0, w0 + BT_W) from the last one down, by wave 0
    const int nwin = (T + BT_W - 1) / BT_W;
    uint32_t wreg[BAND];
    int wave_cur = band_wave(s), wave_next = 0;
    if (wave == 0) {
        load_band(wreg, bp_utt, row_dw, nwin - 1, T, wave_cur * WAVE_DW, lane);
        store_band(wreg, lds.win[(nwin - 1) & 1], lane);
    }
    for (int w = nwin - 1; w >= 0; --w) {
        const int w0 = w * BT_W;
        const int w1 = T - w0 < BT_W ? T : w0 + BT_W;
        if (wave == 0 && w > 0) {  // s is the state at frame w1 - 1: the window below stays within [s - 128, s]
            wave_next = band_wave(s);
            load_band(wreg, bp_utt, row_dw, w - 1, T, wave_next * WAVE_DW, lane);
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t* rows = lds.win[w & 1];
            int mine = -1;
            for (int t = w1 - 1; t >= w0; --t) {
                if (lane == t - w0) mine = s;
                if (t > 0) {  // (row 0 holds no decision: frame 0 is state 0)
                    const uint32_t dw = rows[(t - w0) * BAND + ((s >> 9) - wave_cur) * WAVE_DW + 2 * (s & 7) + ((s >> 8) & 1)];
                    s -= (int)((dw >> ((s >> 3) & 31)) & 1u);
                }
            }
            if (w0 + lane < w1) prow[w0 + lane] = mine;
            if (w > 0) {
                store_band(wreg, lds.win[(w - 1) & 1], lane);
                wave_cur = wave_next;
            }
        }
    }
}

// the dispatcher's table: 512 states per wave
int waves_for(int l_max) { return l_max <= 512 ? 1 : (l_max <= 1024 ? 2 : (l_max <= 2048 ? 4 : (l_max <= 4096 ? 8 : 16))); }

template <int NW>
int launch_align_long(const float* logq, const float* trans, const float* init, const int32_t* labels, const int32_t* label_len,
                      const int32_t* input_len, int32_t* path, float* score, void* workspace, int batch, int t_out, int k,
                      int l_max, hipStream_t s) {
    hipLaunchKernelGGL((asg_align_long_kernel<NW>), dim3(batch), dim3(64 * NW), 0, s, logq, trans, init, labels, label_len,
                       input_len, path, score, (uint32_t*)workspace, t_out, k, l_max);
    return sl_check_launch("sl_asg_align_long");
}

}  // namespace

extern "C" size_t sl_asg_align_long_workspace_bytes(int batch, int t_out, int l_max) {
    if (batch <= 0 || t_out <= 0 || l_max < 1 || l_max > L_LIMIT) return 0;
    return (size_t)batch * t_out * (4 * WAVE_DW * (size_t)waves_for(l_max));
}

extern "C" int sl_asg_align_long(const float* logq, const float* trans, const float* init, const int32_t* labels,
                                 const int32_t* label_len, const int32_t* input_len, int32_t* path, float* score, int batch,
                                 int t_out, int k, int l_max, void* workspace, size_t workspace_bytes, void* stream) {
    SL_CHECK_ARG(batch > 0 && t_out > 0, "sl_asg_align_long: need batch, t_out > 0");
    if (k < 2 || k > 64) {
        sl_set_error("sl_asg_align_long: k = %d outside 2 <= k <= 64 (one staged column per letter)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (l_max < 1 || l_max > L_LIMIT) {
        sl_set_error("sl_asg_align_long: label length %d outside 1 <= l_max <= %d (16 waves of 512 states)", l_max, L_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    SL_CHECK_ARG(logq && trans && init && labels && label_len && input_len && path && score, "sl_asg_align_long: null pointer");
    const size_t need = sl_asg_align_long_workspace_bytes(batch, t_out, l_max);
    SL_CHECK_ARG(workspace, "sl_asg_align_long: workspace is a null pointer");
    if (workspace_bytes < need) {
        sl_set_error("sl_asg_align_long: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
#define SL_ASG_ALIGN_LONG(NW_) \
    return launch_align_long<NW_>(logq, trans, init, labels, label_len, input_len, path, score, workspace, batch, t_out, k, l_max, s)
    switch (waves_for(l_max)) {
        case 1: SL_ASG_ALIGN_LONG(1);
        case 2: SL_ASG_ALIGN_LONG(2);
        case 4: SL_ASG_ALIGN_LONG(4);
        case 8: SL_ASG_ALIGN_LONG(8);
        default: SL_ASG_ALIGN_LONG(16);
    }
#undef SL_ASG_ALIGN_LONG
}
