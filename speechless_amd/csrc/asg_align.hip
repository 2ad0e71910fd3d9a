// asg_align.hip -- ASG forced alignment (Viterbi over a label's own states under emissions + transition scores, and the
// backtrace) for gfx950: the segmentation the auto segmentation criterion is named for.
//
// No reference counterpart: the reference only CONSUMES word timings (speechless/labeled_example.py:32-60, 219-234) and has no
// ASG at all (speechless/net.py:397-399).  Semantics (bit for bit, fp32): include/speechless_hip.h, sl_asg_align.
//
// Kernel asg_align_kernel<NS, BP_LDS>: ONE WAVE per utterance, NS consecutive states per lane in registers (lane l holds
// states l*NS .. l*NS + NS - 1; NS = 1 / 2 / 4 / 8 for l_max <= 64 / 128 / 256 / 511, as asg_lattice_kernel<NS> picks).  A
// lane gathers the column of each of its states and the two scores it ever needs, g(l_s, l_s) and g(l_{s-1}, l_s), once.  Per
// frame: the highest state of the lane below arrives by one DPP wave_shr:1 move, every state takes stay = d(s) + g(l_s, l_s)
// and move = d(s-1) + g(l_{s-1}, l_s), keeps the larger (stay on a tie) and adds its emission -- three separately rounded
// adds and an exact max: there is no multiply, so no FMA can form (asg_frame of lattice.h, which asg_align_long.hip runs too). 
// The compare of state j of every lane IS the frame's backpointer word j (a 64-bit lane mask): one bit per state and frame, rows
// of NS words = 8*NS bytes, state s at bit s / NS of word s % NS.  Emissions come from LDS: the wave stages ALIGN_CH frames of
// logq rows (k <= 64 floats, one coalesced read per frame) while it works on the previous ALIGN_CH frames (EmissionStager of
// lattice.h).
//   BP_LDS = 1: the T' rows fit the work-group's LDS (config 3: 500 frames x 16 bytes) and the backtrace reads them there.
//   BP_LDS = 0: rows go to the workspace in HBM; the backtrace copies windows of BT_W frames into LDS, the next window's
//   loads in flight while the current one is resolved (lattice.h, as ctc_align.hip does).
// The backtrace is run by every lane of the wave on the same (wave-uniform) state: its LDS reads are broadcasts, and lane
// t - w0 keeps the state of frame t, so the path leaves as one coalesced store per window.
#include <math.h>

#include "lattice.h"

namespace {

__host__ __device__ constexpr int row_bytes(int ns) { return 8 * ns; }  // ns lane masks of 64 bits

// LDS: [logq chunk ALIGN_CH x 64 floats][final scores 64*NS floats][backpointer rows: T' rows (BP_LDS) or two windows of BT_W rows]
template <int NS, bool BP_LDS>
__global__ __launch_bounds__(64) void asg_align_kernel(const float* __restrict__ logq, const float* __restrict__ trans,
                                                        const float* __restrict__ init, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ label_len,
                                                        const int32_t* __restrict__ input_len, int32_t* __restrict__ path,
                                                        float* __restrict__ score, uint8_t* __restrict__ bp_hbm, int t_out,
                                                        int k, int l_max) {
    constexpr int R = row_bytes(NS);
    extern __shared__ float smem[];
    float* em = smem;
    float* fin = em + ALIGN_CH * 64;
    uint8_t* rows = (uint8_t*)(fin + 64 * NS);

    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    const int32_t* lab = labels + (long)b * l_max;
    int32_t* prow = path + (long)b * t_out;

    for (int t = T + lane; t < t_out; t += 64) prow[t] = -1;
    if (L == 0 || T == 0 || L > T) {  // infeasible, as sl_asg_loss_grad decides
        for (int t = lane; t < T; t += 64) prow[t] = -1;
        if (lane == 0) score[b] = -INFINITY;
        return;
    }

    // per-lane states: lane l holds states l*NS .. l*NS + NS - 1 with their emission column, stay score and move score (lattice.h)
    int col[NS];
    float gs[NS], ga[NS], d[NS];
    asg_states_init<NS>(col, gs, ga, lab, lane * NS, L, k, trans);
    const float* lq = logq + (long)b * t_out * k;
    // frame 0: only state 0 is open (here and not in a helper: see asg_states_init)
#pragma unroll
    for (int j = 0; j < NS; ++j) d[j] = lane * NS + j == 0 ? init[col[0]] + lq[col[0]] : -INFINITY;

    EmissionStager<64> stg;
    stg.prefetch(lq, 1, T, k, 0, lane);  // chunks start at frame 1
    uint64_t* bp_rows = BP_LDS ? (uint64_t*)rows : (uint64_t*)(bp_hbm + (long)b * t_out * R);
    for (int t0 = 1; t0 < T; t0 += ALIGN_CH) {
        __syncthreads();
        stg.store(em, 0, lane);
        __syncthreads();
        if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, 0, lane);
        const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
#pragma unroll
        for (int f = 0; f < ALIGN_CH; ++f) {
            if (f >= nf) continue;  // (wave-uniform; a break keeps the loop from unrolling)
            const float lo = dpp_float_from_lower_lane(d[NS - 1], -INFINITY);  // state lane*NS - 1
            uint64_t word[NS];
            asg_frame<NS>(col, gs, ga, d, em + f * 64, lo, word);
            if (lane == 0) {
                uint64_t* row = bp_rows + (long)(t0 + f) * NS;
#pragma unroll
                for (int j = 0; j < NS; ++j) row[j] = word[j];
            }
        }
    }

    // end state L - 1
#pragma unroll
    for (int j = 0; j < NS; ++j) fin[lane * NS + j] = d[j];
    if (!BP_LDS) __threadfence();
    __syncthreads();
    const float best = fin[L - 1];
    if (lane == 0) score[b] = best;
    if (best == -INFINITY) {  // -inf scores closed every path
        for (int t = lane; t < T; t += 64) prow[t] = -1;
        return;
    }
    int s = L - 1;

    // backtrace, windows [w0, w0 + BT_W) from the last one down
    const int nwin = (T + BT_W - 1) / BT_W;
    constexpr int VR = BP_LDS ? 1 : NS;  // u32x2 per lane of one window: BT_W * R / 8 / 64 (none when the rows stay in LDS)
    u32x2 wreg[VR];
    const uint8_t* bp_utt = bp_hbm + (long)b * t_out * R;
    if (!BP_LDS) {
        load_window<u32x2, VR, R>(wreg, bp_utt, nwin - 1, T, lane);
        store_window<u32x2, VR, R>(wreg, rows, nwin - 1, lane);
    }
    for (int w = nwin - 1; w >= 0; --w) {
        const int w0 = w * BT_W;
        const int w1 = T - w0 < BT_W ? T : w0 + BT_W;
        if (!BP_LDS && w > 0) load_window<u32x2, VR, R>(wreg, bp_utt, w - 1, T, lane);
        __syncthreads();
        const uint64_t* base = (const uint64_t*)(BP_LDS ? rows + (long)w0 * R : rows + (w & 1) * BT_W * R);
        int mine = -1;
        for (int t = w1 - 1; t >= w0; --t) {
            if (lane == t - w0) mine = s;
            if (t > 0) s -= (int)((base[(t - w0) * NS + (s % NS)] >> (s / NS)) & 1u);
        }
        if (w0 + lane < w1) prow[w0 + lane] = mine;
        if (!BP_LDS && w > 0) {
            __syncthreads();
            store_window<u32x2, VR, R>(wreg, rows, w - 1, lane);
        }
    }
}

size_t align_lds_bytes(int ns, bool bp_lds, int t_out) {
    return (size_t)(ALIGN_CH * 64 + 64 * ns) * sizeof(float) + (size_t)(bp_lds ? t_out : 2 * BT_W) * row_bytes(ns);
}

int states_per_lane(int l_max) { return l_max <= 64 ? 1 : (l_max <= 128 ? 2 : (l_max <= 256 ? 4 : 8)); }

template <int NS, bool BP_LDS>
int launch_align(const float* logq, const float* trans, const float* init, const int32_t* labels, const int32_t* label_len,
                 const int32_t* input_len, int32_t* path, float* score, void* workspace, int batch, int t_out, int k, int l_max,
                 hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)asg_align_kernel<NS, BP_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   ALIGN_LDS_MAX);
        attr_set = true;
    }
    hipLaunchKernelGGL((asg_align_kernel<NS, BP_LDS>), dim3(batch), dim3(64), align_lds_bytes(NS, BP_LDS, t_out), s, logq, trans,
                       init, labels, label_len, input_len, path, score, (uint8_t*)workspace, t_out, k, l_max);
    return sl_check_launch("sl_asg_align");
}

}  // namespace

extern "C" size_t sl_asg_align_workspace_bytes(int batch, int t_out, int l_max) {
    if (batch <= 0 || t_out <= 0 || l_max < 1 || l_max > 511) return 0;
    const int ns = states_per_lane(l_max);
    return align_lds_bytes(ns, true, t_out) <= (size_t)ALIGN_LDS_MAX ? 0 : (size_t)batch * t_out * row_bytes(ns);
}

extern "C" int sl_asg_align(const float* logq, const float* trans, const float* init, const int32_t* labels,
                            const int32_t* label_len, const int32_t* input_len, int32_t* path, float* score, int batch, int t_out,
                            int k, int l_max, void* workspace, size_t workspace_bytes, void* stream) {
    SL_CHECK_ARG(batch > 0 && t_out > 0, "sl_asg_align: need batch, t_out > 0");
    if (k < 2 || k > 64) {
        sl_set_error("sl_asg_align: k = %d outside 2 <= k <= 64 (one lane per letter)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (l_max < 1 || l_max > 511) {
        sl_set_error("sl_asg_align: label length %d outside 1 <= l_max <= 511 (at most 8 states per lane)", l_max);
        return SL_ERR_UNSUPPORTED;
    }
    SL_CHECK_ARG(logq && trans && init && labels && label_len && input_len && path && score, "sl_asg_align: null pointer");
    const size_t need = sl_asg_align_workspace_bytes(batch, t_out, l_max);
    if (workspace_bytes < need || (need > 0 && workspace == nullptr)) {
        sl_set_error("sl_asg_align: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
    const bool lds = need == 0;
#define SL_ASG_ALIGN(NS_)                                                                                                     \
    return lds ? launch_align<NS_, true>(logq, trans, init, labels, label_len, input_len, path, score, workspace, batch, t_out, \
                                         k, l_max, s)                                                                         \
               : launch_align<NS_, false>(logq, trans, init, labels, label_len, input_len, path, score, workspace, batch,      \
                                          t_out, k, l_max, s)
    switch (states_per_lane(l_max)) {
        case 1: SL_ASG_ALIGN(1);
        case 2: SL_ASG_ALIGN(2);
        case 4: SL_ASG_ALIGN(4);
        default: SL_ASG_ALIGN(8);
    }
#undef SL_ASG_ALIGN
}
