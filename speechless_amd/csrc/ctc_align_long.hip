// ctc_align_long.hip -- CTC forced alignment of LONG recordings: sl_ctc_align (ctc_align.hip) beyond 511 letters, for gfx950.
//
// The aligners exist to produce the word timings with which LabeledExampleFromFile.sections() (speechless/labeled_example.py:
// 219-234) cuts long recordings; a ten-minute recording has thousands of letters.  Semantics (bit for bit, fp32): those of
// sl_ctc_align, include/speechless_hip.h.  Only the limits differ: l_max <= 8191 (16 383 lattice states).
//
// Kernel ctc_align_long_kernel<NW>: ONE WORK-GROUP of NW waves (1 / 2 / 4 / 8 / 16 for l_max <= 511 / 1023 / 2047 / 4095 /
// 8191) per recording, 16 consecutive lattice states per lane in registers: thread i holds states 16 i .. 16 i + 15.  A
// thread's first state is a blank (never skips), so per frame exactly one value crosses a thread boundary: the highest state of
// the thread below.  Inside a wave it moves by the DPP wave_shr:1 of lattice.h; across waves it goes through one LDS slot per
// wave, double-buffered by frame parity (lane 63 of wave w writes slot [t & 1][w] after frame t, lane 0 of wave w + 1 reads it
// in frame t + 1), which costs ONE work-group barrier per frame.  Every barrier is uniform: all trip counts depend on the
// recording only.  Per state and frame: max(stay, s-1, s-2) with the strict-> tie rule and ONE rounded add (no multiply: nothing
// to contract) -- ctc_frame of lattice.h, the very step of ctc_align.hip.  Emissions come from LDS: the work-group stages
// ALIGN_CH frames of logq rows (k <= 64 floats) once for all waves while the next ALIGN_CH frames are in flight in registers
// (EmissionStager of lattice.h, with all NW waves at work).
// Backpointers: 2 bits per state and frame, a thread's 16 states = one dword, a frame's row = 256 NW bytes stored coalesced to
// the workspace in HBM (state s at bits 2 (s & 15) of dword s >> 4).
// Backtrace: wave 0 (the other waves only keep the barriers uniform).  The path drops at most two states per frame, so a window
// of BT_W = 64 frames whose top frame is at state s touches states [s - 128, s] only, and the window below it [s - 256, s]: 17
// dwords of each row.  That band of the NEXT window is loaded into registers (load_band / store_band of lattice.h) before the
// current window is resolved out of LDS, so no step of the T'-long chain waits on a dependent HBM load.  Lane t - w0 keeps frame
// t's state: one coalesced store per window.
#include "lattice.h"

namespace {

constexpr int NJ = 16;       // lattice states per thread
constexpr int BAND = 17;     // backpointer dwords of a row that two windows below a state can touch (2 * 2 * BT_W / NJ + 1)
constexpr int L_LIMIT = 8191;

// LDS: [logq chunk ALIGN_CH x 64 floats][boundary slots 2 x 16][reduction 16 ints][end scores 2]
//      [backtrace windows 2 x BT_W x BAND dwords]
struct LongLds {
    float em[ALIGN_CH * 64];
    float edge[2][16];
    int reps[16];
    float fin[2];
    uint32_t win[2][BT_W * BAND];
};

__device__ __forceinline__ int band_base(int s) { return s > 256 ? (s - 256) >> 4 : 0; }  // first dword of [s - 256, s]

template <int NW>
__global__ __launch_bounds__(64 * NW) void ctc_align_long_kernel(const float* __restrict__ logq, const int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ label_len,
                                                                 const int32_t* __restrict__ input_len, int32_t* __restrict__ path,
                                                                 float* __restrict__ score, uint32_t* __restrict__ bp_hbm, int t_out,
                                                                 int k, int l_max) {
    constexpr int NT = 64 * NW;        // threads = dwords of a backpointer row
    __shared__ LongLds lds;

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int blank = k - 1;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    const int S = 2 * L + 1;
    const int32_t* lab = labels + (long)b * l_max;
    int32_t* prow = path + (long)b * t_out;

    // feasibility: T >= L + (adjacent equal labels)
    int reps = 0;
    for (int i0 = 1; i0 < L; i0 += NT) {
        const int i = i0 + tid;
        const bool eq = i < L && lab[i] == lab[i - 1];
        reps += __popcll(__ballot(eq));
    }
    if (lane == 0) lds.reps[wave] = reps;
    if (tid < 32) lds.edge[tid >> 4][tid & 15] = -INFINITY;  // the virtual frame -1: nothing below any wave
    __syncthreads();
    reps = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) reps += lds.reps[w];
    for (int t = T + tid; t < t_out; t += NT) prow[t] = -1;
    if (T < L + reps || T == 0) {  // (uniform over the work-group: no barrier follows)
        for (int t = tid; t < T; t += NT) prow[t] = -1;
        if (tid == 0) score[b] = (T == 0 && L == 0) ? 0.f : -INFINITY;
        return;
    }

    // per-thread lattice: thread i holds states 16 i .. 16 i + 15, at the virtual frame -1 (lattice.h)
    int col[NJ / 2];
    bool skip[NJ / 2];
    float d[NJ];
    ctc_states_init<NJ>(col, skip, lab, tid * NJ, S, k);
    // delta of a virtual frame -1: state 0 at 0, the rest at -inf, so that frame 0 yields delta_0(0) = logq_0(blank) and
    // delta_0(1) = logq_0(l_0) exactly (0 + x == x) and every other state -inf
#pragma unroll
    for (int j = 0; j < NJ; ++j) d[j] = tid * NJ + j == 0 ? 0.f : -INFINITY;

    const float* lq = logq + (long)b * t_out * k;
    EmissionStager<NT> stg;
    stg.prefetch(lq, 0, T, k, wave, lane);
    const int row_dw = NT;
    uint32_t* bp_utt = bp_hbm + (long)b * t_out * row_dw;
    for (int t0 = 0; t0 < T; t0 += ALIGN_CH) {
        // (the barrier that ended the previous chunk's last frame: every wave is done with the old rows)
        stg.store(lds.em, wave, lane);
        __syncthreads();
        if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, wave, lane);
        const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
#pragma unroll
        for (int f = 0; f < ALIGN_CH; ++f) {
            if (f >= nf) continue;  // (uniform over the work-group; a break keeps the loop from unrolling)
            const int t = t0 + f;
            const float* e = lds.em + f * 64;
            // state 16 tid - 1: s-1 of the thread's first state (even: never skips) and s-2 of its second
            float lo1 = dpp_float_from_lower_lane(d[NJ - 1], -INFINITY);
            if (NW > 1 && lane == 0 && wave > 0) lo1 = lds.edge[(t + 1) & 1][wave - 1];  // written after frame t - 1
            const uint32_t word = ctc_frame<NJ>(col, skip, d, e, e[blank], lo1);
            if (NW > 1 && lane == 63) lds.edge[t & 1][wave] = d[NJ - 1];
            bp_utt[(long)t * row_dw + tid] = word;
            __syncthreads();  // the frame's barrier: boundary slots written, and (last frame of a chunk) the rows read
        }
    }

    // end state: the better of S-1 and S-2, S-1 on a tie
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (tid * NJ + j == S - 1) lds.fin[1] = d[j];
        if (tid * NJ + j == S - 2) lds.fin[0] = d[j];
    }
    __syncthreads();  // also orders every wave's backpointer rows before wave 0 reads them
    int s = S - 1;
    if (S >= 2 && lds.fin[0] > lds.fin[1]) s = S - 2;
    if (tid == 0) score[b] = lds.fin[s == S - 1 ? 1 : 0];

    // backtrace, windows [w0, w0 + BT_W) from the last one down, by wave 0
    const int nwin = (T + BT_W - 1) / BT_W;
    uint32_t wreg[BAND];
    int base_cur = band_base(s), base_next = 0;
    if (wave == 0) {
        load_band(wreg, bp_utt, row_dw, nwin - 1, T, base_cur, lane);
        store_band(wreg, lds.win[(nwin - 1) & 1], lane);
    }
    for (int w = nwin - 1; w >= 0; --w) {
        const int w0 = w * BT_W;
        const int w1 = T - w0 < BT_W ? T : w0 + BT_W;
        if (wave == 0 && w > 0) {  // s is the state at frame w1 - 1: the window below stays within [s - 256, s]
            base_next = band_base(s);
            load_band(wreg, bp_utt, row_dw, w - 1, T, base_next, lane);
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t* rows = lds.win[w & 1];
            int mine = -1;
            for (int t = w1 - 1; t >= w0; --t) {
                if (lane == t - w0) mine = s;
                if (t > 0) {
                    const uint32_t dw = rows[(t - w0) * BAND + (s >> 4) - base_cur];
                    s -= (dw >> (2 * (s & 15))) & 3u;
                }
            }
            if (w0 + lane < w1) prow[w0 + lane] = mine;
            if (w > 0) {
                store_band(wreg, lds.win[(w - 1) & 1], lane);
                base_cur = base_next;
            }
        }
    }
}

int waves_for(int l_max) { return l_max <= 511 ? 1 : (l_max <= 1023 ? 2 : (l_max <= 2047 ? 4 : (l_max <= 4095 ? 8 : 16))); }

template <int NW>
int launch_align_long(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len, int32_t* path,
                      float* score, void* workspace, int batch, int t_out, int k, int l_max, hipStream_t s) {
    hipLaunchKernelGGL((ctc_align_long_kernel<NW>), dim3(batch), dim3(64 * NW), 0, s, logq, labels, label_len, input_len, path,
                       score, (uint32_t*)workspace, t_out, k, l_max);
    return sl_check_launch("sl_ctc_align_long");
}

}  // namespace

extern "C" size_t sl_ctc_align_long_workspace_bytes(int batch, int t_out, int l_max) {
    if (batch <= 0 || t_out <= 0 || l_max < 0 || l_max > L_LIMIT) return 0;
    return (size_t)batch * t_out * (256 * (size_t)waves_for(l_max));
}

extern "C" int sl_ctc_align_long(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len,
                                 int32_t* path, float* score, int batch, int t_out, int k, int l_max, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    SL_CHECK_ARG(batch > 0 && t_out > 0 && l_max >= 0, "sl_ctc_align_long: need batch, t_out > 0 and l_max >= 0");
    SL_CHECK_ARG(logq, "sl_ctc_align_long: logq is a null pointer");
    SL_CHECK_ARG(labels || l_max == 0, "sl_ctc_align_long: labels is a null pointer (l_max = %d)", l_max);
    SL_CHECK_ARG(label_len, "sl_ctc_align_long: label_len is a null pointer");
    SL_CHECK_ARG(input_len, "sl_ctc_align_long: input_len is a null pointer");
    SL_CHECK_ARG(path, "sl_ctc_align_long: path is a null pointer");
    SL_CHECK_ARG(score, "sl_ctc_align_long: score is a null pointer");
    if (k <= 1 || k > 64) {
        sl_set_error("sl_ctc_align_long: k = %d outside 1 < k <= 64 (one staged column per class)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (l_max > L_LIMIT) {
        sl_set_error("sl_ctc_align_long: l_max = %d > %d unsupported (at most 16383 lattice states)", l_max, L_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    const size_t need = sl_ctc_align_long_workspace_bytes(batch, t_out, l_max);
    if (workspace_bytes < need || workspace == nullptr) {
        sl_set_error("sl_ctc_align_long: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
#define SL_ALIGN_LONG(NW_) \
    return launch_align_long<NW_>(logq, labels, label_len, input_len, path, score, workspace, batch, t_out, k, l_max, s)
    switch (waves_for(l_max)) {
        case 1: SL_ALIGN_LONG(1);
        case 2: SL_ALIGN_LONG(2);
        case 4: SL_ALIGN_LONG(4);
        case 8: SL_ALIGN_LONG(8);
        default: SL_ALIGN_LONG(16);
    }
#undef SL_ALIGN_LONG
}
