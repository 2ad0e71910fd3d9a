// ctc_segment.hip -- CTC segment posteriors for gfx950: the probability that a stretch of frames, read on its own, says exactly
// a stretch of a label (the forward sum over the CTC lattice of those letters and those frames).  With the word ranges of a
// forced alignment it is a per-word confidence; over a section of a long recording it is what tells a section whose transcript
// does not match its audio from one that does.
//
// No reference counterpart: the reference's sections() (speechless/labeled_example.py:219-234) takes its word timings on trust.
// Semantics: include/speechless_hip.h, sl_ctc_segment_scores.
//
// Kernel ctc_segment_kernel<NJ>: ONE WAVE per segment in a work-group of 64 threads, NJ consecutive lattice states per lane in
// registers (lane l holds states l*NJ .. l*NJ + NJ - 1; NJ = 2 / 4 / 8 / 16 for segments of up to 63 / 127 / 255 / 511 letters:
// words take the smallest, sections of a recording the larger ones).  The states, their label columns and skip flags, the
// neighbour-lane move and the emission stager are those of the aligners (lattice.h); only the frame step differs: it SUMS where
// theirs takes the max (ctc_frame_sum), in doubles and log2 units with the fp32 exp2 / log2 step of ctc_long.hip (lse_double.h),
// and it keeps no backpointers.  The wave stages ALIGN_CH frames of logq rows, starting at the segment's first frame, while it
// works on the previous ALIGN_CH.  Nothing is written but the segment's float.
#include "lattice.h"

namespace {

constexpr int SEG_L_LIMIT = 511;

__device__ __forceinline__ int clamp_range(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int NJ>
__global__ __launch_bounds__(64) void ctc_segment_kernel(const float* __restrict__ logq, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ input_len,
                                                          const int32_t* __restrict__ segments, float* __restrict__ out, int batch,
                                                          int t_out, int k, int l_max, int seg_l_max) {
    __shared__ float em[ALIGN_CH * 64];
    __shared__ double fin[2];  // the last frame's states S-2 and S-1

    const int lane = threadIdx.x;
    const int32_t* sg = segments + (long)blockIdx.x * 5;
    float* res = out + blockIdx.x;
    const int b = sg[0];
    if (b < 0 || b >= batch) {  // (every exit before the frames is uniform over the wave: no barrier has been met)
        if (lane == 0) *res = -INFINITY;
        return;
    }
    const int Tb = clamp_range(input_len[b], t_out);
    const int f0 = clamp_range(sg[1], Tb);
    const int f1 = clamp_range(sg[2], Tb);
    const int T = f1 > f0 ? f1 - f0 : 0;
    const int l0 = clamp_range(sg[3], l_max);
    const int l1 = clamp_range(sg[4], l_max);
    int L = l1 > l0 ? l1 - l0 : 0;
    L = L > seg_l_max ? seg_l_max : L;
    const int S = 2 * L + 1;
    const int blank = k - 1;
    const int32_t* lab = labels + (long)b * l_max + l0;

    // feasibility: T >= L + (adjacent equal labels)
    int reps = 0;
    for (int i0 = 1; i0 < L; i0 += 64) {
        const int i = i0 + lane;
        const bool eq = i < L && lab[i] == lab[i - 1];
        reps += __popcll(__ballot(eq));
    }
    if (T < L + reps || T == 0) {
        if (lane == 0) *res = (T == 0 && L == 0) ? 0.f : -INFINITY;
        return;
    }

    // per-lane lattice: lane l holds states l*NJ .. l*NJ + NJ - 1, at the virtual frame -1 (lattice.h)
    int col[NJ / 2];
    bool skip[NJ / 2];
    double d[NJ];
    ctc_states_init<NJ>(col, skip, lab, lane * NJ, S, k);
    // alpha of a virtual frame -1: state 0 at 0, the rest at -inf, so that frame 0 yields a_0(0) = logq_0(blank) and
    // a_0(1) = logq_0(l_0) (log2(2^0 + 0) == 0 exactly) and every other state -inf
#pragma unroll
    for (int j = 0; j < NJ; ++j) d[j] = lane * NJ + j == 0 ? 0.0 : NEG_INF_D;
    if (lane < 2) fin[lane] = NEG_INF_D;  // (S == 1 has no state S-2; ordered before the reads by the barriers of the first chunk)

    const float* lq = logq + ((long)b * t_out + f0) * k;  // rows f0 .. f0 + T - 1: inside [0, Tb) of utterance b
    EmissionStager<64> stg;
    stg.prefetch(lq, 0, T, k, 0, lane);
    for (int t0 = 0; t0 < T; t0 += ALIGN_CH) {
        __syncthreads();
        stg.store(em, 0, lane);
        __syncthreads();
        if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, 0, lane);
        const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
#pragma unroll
        for (int f = 0; f < ALIGN_CH; ++f) {
            if (f >= nf) continue;  // (wave-uniform; a break keeps the loop from unrolling)
            const float* e = em + f * 64;
            // state lane*NJ - 1: s-1 of the lane's first state (even: never skips) and s-2 of its second
            const double lo1 = dpp_double_from_lower_lane(d[NJ - 1], NEG_INF_D);
            ctc_frame_sum<NJ>(col, skip, d, e, e[blank], lo1);
        }
    }

    // result: log(2^a(S-1) + 2^a(S-2)) in nats
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (lane * NJ + j == S - 1) fin[1] = d[j];
        if (lane * NJ + j == S - 2) fin[0] = d[j];
    }
    __syncthreads();
    if (lane == 0) *res = (float)(lse2_long(fin[0], fin[1]) * LN2_D);
}

int states_per_lane(int seg_l_max) { return seg_l_max <= 63 ? 2 : (seg_l_max <= 127 ? 4 : (seg_l_max <= 255 ? 8 : 16)); }

template <int NJ>
int launch_segment(const float* logq, const int32_t* labels, const int32_t* input_len, const int32_t* segments, float* out,
                   int batch, int t_out, int k, int l_max, int n_segments, int seg_l_max, hipStream_t s) {
    hipLaunchKernelGGL((ctc_segment_kernel<NJ>), dim3(n_segments), dim3(64), 0, s, logq, labels, input_len, segments, out, batch,
                       t_out, k, l_max, seg_l_max);
    return sl_check_launch("sl_ctc_segment_scores");
}

}  // namespace

extern "C" size_t sl_ctc_segment_scores_workspace_bytes(int n_segments, int seg_l_max) {
    (void)n_segments;
    (void)seg_l_max;
    return 0;  // the lattice of a segment lives in its wave's registers
}

extern "C" int sl_ctc_segment_scores(const float* logq, const int32_t* labels, const int32_t* input_len, const int32_t* segments,
                                     float* log_posterior, int batch, int t_out, int k, int l_max, int n_segments, int seg_l_max,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (k <= 1 || k > 64) {
        sl_set_error("sl_ctc_segment_scores: k = %d outside 1 < k <= 64 (one lane per class)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (seg_l_max < 0 || seg_l_max > SEG_L_LIMIT) {
        sl_set_error("sl_ctc_segment_scores: seg_l_max = %d outside 0 <= seg_l_max <= %d (at most 1023 lattice states per segment)",
                     seg_l_max, SEG_L_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    if (n_segments < 1) {
        sl_set_error("sl_ctc_segment_scores: n_segments = %d, need n_segments >= 1", n_segments);
        return SL_ERR_UNSUPPORTED;
    }
    SL_CHECK_ARG(batch > 0 && t_out > 0 && l_max >= 0, "sl_ctc_segment_scores: need batch, t_out > 0 and l_max >= 0");
    SL_CHECK_ARG(logq, "sl_ctc_segment_scores: logq is a null pointer");
    SL_CHECK_ARG(labels || l_max == 0, "sl_ctc_segment_scores: labels is a null pointer (l_max = %d)", l_max);
    SL_CHECK_ARG(input_len, "sl_ctc_segment_scores: input_len is a null pointer");
    SL_CHECK_ARG(segments, "sl_ctc_segment_scores: segments is a null pointer");
    SL_CHECK_ARG(log_posterior, "sl_ctc_segment_scores: log_posterior is a null pointer");
    const size_t need = sl_ctc_segment_scores_workspace_bytes(n_segments, seg_l_max);
    if (workspace_bytes < need || (need > 0 && workspace == nullptr)) {
        sl_set_error("sl_ctc_segment_scores: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
#define SL_SEGMENT(NJ_) \
    return launch_segment<NJ_>(logq, labels, input_len, segments, log_posterior, batch, t_out, k, l_max, n_segments, seg_l_max, s)
    switch (states_per_lane(seg_l_max)) {
        case 2: SL_SEGMENT(2);
        case 4: SL_SEGMENT(4);
        case 8: SL_SEGMENT(8);
        default: SL_SEGMENT(16);
    }
#undef SL_SEGMENT
}
