// asg_segment.hip -- ASG segment posteriors for gfx950: the probability that a stretch of frames says exactly a stretch of an
// encoded label under the auto segmentation criterion -- the forward sum over the label's own states (constrained) minus the
// forward sum over the full graph of k graphemes (free), both over the segment's frames and from the same start scores.  ASG is
// globally normalised, so the difference is the log of a proper probability; over the whole label and all frames it is minus
// the ASG loss.  The ASG twin of ctc_segment.hip: with the word ranges of sl_asg_align a per-word confidence, over a section of
// a long recording the check whether the section's transcript matches its audio.
//
// No reference counterpart (the reference has no ASG at all: speechless/net.py:397-399).
// Semantics: include/speechless_hip.h, sl_asg_segment_scores.
//
// Kernel asg_segment_kernel<NS>: one work-group of TWO WAVES per segment.  The two recursions are independent until the final
// subtraction, so they run side by side on the same staged emissions: every ALIGN_CH frames both waves stage the next chunk of
// logq rows (EmissionStager<128> of lattice.h, starting at the segment's first frame, prefetched one chunk ahead).
//   wave 0  numerator: NS consecutive states per lane in registers (lane l holds states l*NS .. l*NS + NS - 1; NS = 1 / 2 / 4 /
//           8 for segments of up to 64 / 128 / 256 / 511 graphemes), in doubles and the LOG domain (log2 units) -- asg.hip's
//           header says why the probability domain loses collapsed utterances here.  States and columns are the aligners'
//           (asg_states_init), the neighbour comes by dpp_double_from_lower_lane, the frame step is asg_frame_sum of lattice.h.
//   wave 1  denominator: lane j owns grapheme j, in doubles and the PROBABILITY domain, the scheme of asg_lattice_kernel's
//           role 2: exp(g) is computed once by both waves into LDS as [from][to] (a lane's reads of one row are consecutive:
//           conflict-free) and the lane's column moves from there into KR = 32 / 64 registers (k <= 32 / 64); a frame is k
//           multiply-adds per lane against the previous frame's values and one rescale.  The wave's frames are a dependent
//           chain, so nothing that can be had elsewhere sits on it: the previous values go through LDS once and come back as
//           broadcast reads that are all in flight together, the rescale is by the power of two of the previous frame's
//           largest value, which every lane finds among those values (no reduction, no division, exact), and log Z is the
//           sum of those exponents times ln 2 plus ONE log of the last frame's sum.  The
//           frame's largest emission is subtracted before the exp and added back to log Z, a chunk of frames at a time ahead
//           of the chain, so a finite logq row of any magnitude works and a frame whose sum is 0 gives Z = -inf.
// Nothing is written but the segment's float.
#include <math.h>

#include "lattice.h"

namespace {

constexpr int SEG_L_LIMIT = 511;

__device__ __forceinline__ int clamp_range(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the largest value of the wave in every lane, without LDS: two quad permutes and two mirrors leave each row of 16 lanes with
// its maximum, four lane reads fetch the rows' (ds_bpermute shuffles cost an LDS round trip per step)
__device__ __forceinline__ float wave_max_f(float v) {
#define SL_DPP_MAX(CTRL_) \
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL_, 0xf, 0xf, false)))
    SL_DPP_MAX(0xB1);   // quad_perm [1, 0, 3, 2]
    SL_DPP_MAX(0x4E);   // quad_perm [2, 3, 0, 1]
    SL_DPP_MAX(0x141);  // row_half_mirror
    SL_DPP_MAX(0x140);  // row_mirror
#undef SL_DPP_MAX
    const int r = __float_as_int(v);
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(r, 0)), __int_as_float(__builtin_amdgcn_readlane(r, 16))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(r, 32)), __int_as_float(__builtin_amdgcn_readlane(r, 48))));
}

// dynamic LDS: 64 doubles of the denominator's previous frame (first: 16-byte aligned), [k][k] doubles exp(g) as [from][to],
// 2 doubles N and log Z, then the chunk of ALIGN_CH x 64 floats
__host__ __device__ constexpr size_t segment_lds_bytes(int k) {
    return (size_t)(64 + k * k + 2) * sizeof(double) + (size_t)ALIGN_CH * 64 * sizeof(float);
}

template <int NS, int KR>
__global__ __launch_bounds__(128) void asg_segment_kernel(const float* __restrict__ logq, const float* __restrict__ trans,
                                                           const float* __restrict__ init, const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ input_len,
                                                           const int32_t* __restrict__ segments, float* __restrict__ out,
                                                           int batch, int t_out, int k, int l_max, int seg_l_max) {
    extern __shared__ double smem_d[];
    double* vec = smem_d;
    double* G = vec + 64;
    double* fin = G + k * k;  // [0] N in log2 units, [1] log Z in nats
    float* em = (float*)(fin + 2);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t* sg = segments + (long)blockIdx.x * 5;
    float* res = out + blockIdx.x;
    const int b = sg[0];
    if (b < 0 || b >= batch) {  // (every exit before the frames is uniform over the work-group: no barrier has been met)
        if (threadIdx.x == 0) *res = -INFINITY;
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
    if (L == 0 || T < L) {  // without a blank no path says nothing; a state takes a frame at least
        if (threadIdx.x == 0) *res = (T == 0 && L == 0) ? 0.f : -INFINITY;
        return;
    }
    const int32_t* lab = labels + (long)b * l_max + l0;
    // start scores s(j): g0 at the label's begin, else the move out of the grapheme the label puts before the segment
    const float* start = l0 == 0 ? init : trans + clamp_label(lab[-1], k) * k;

    for (int idx = threadIdx.x; idx < k * k; idx += 128) G[idx] = exp((double)trans[idx]);  // (-inf -> 0)

    // wave 0: per-lane states with their emission column, stay score and move score (lattice.h), the scores in log2 units
    int col[NS];
    double gs[NS], ga[NS], d[NS];
    {
        float gsf[NS], gaf[NS];
        asg_states_init<NS>(col, gsf, gaf, lab, lane * NS, L, k, trans);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            gs[j] = (double)gsf[j] * LOG2E_D;
            ga[j] = (double)gaf[j] * LOG2E_D;  // (state 0's stays -inf)
            d[j] = NEG_INF_D;                  // frame 0 opens state 0 (below: the kernel itself, see asg_states_init)
        }
    }
    const double s0 = (double)start[col[0]] * LOG2E_D;  // (read by lane 0 only, whose col[0] is l_0)
    // wave 1: lane j owns grapheme j
    const bool on = lane < k;
    const int lj = on ? lane : 0;
    const double sj = on ? exp((double)start[lj]) : 0.0;
    // its column of exp(g) in registers: gcol[i] = exp(g(i, j)), zeros past k.  (Both waves load it: the branch between the waves
    // is no reason for the compiler to keep two register files apart, and an array half initialised buys nothing.)
    double gcol[KR];
    __syncthreads();  // G is filled (uniform: every thread of a segment that has frames arrives here)
#pragma unroll
    for (int i = 0; i < KR; ++i) gcol[i] = i < k ? G[i * k + lj] : 0.0;
    double v = 0.0, msum = 0.0;  // the frame's values; the sum of the emission maxima taken out
    int esum = 0;                // the sum of the binary exponents taken out

    const float* lq = logq + ((long)b * t_out + f0) * k;  // rows f0 .. f0 + T - 1: inside [0, Tb) of utterance b
    EmissionStager<128> stg;
    stg.prefetch(lq, 0, T, k, wave, lane);
    for (int t0 = 0; t0 < T; t0 += ALIGN_CH) {
        __syncthreads();
        stg.store(em, wave, lane);
        __syncthreads();
        if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, wave, lane);
        const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
        if (wave == 0) {
#pragma unroll
            for (int f = 0; f < ALIGN_CH; ++f) {
                if (f >= nf) continue;  // (wave-uniform; a break keeps the loop from unrolling)
                const float* e = em + f * 64;
                if (f == 0 && t0 == 0) {
                    if (lane == 0) d[0] = fma((double)e[col[0]], LOG2E_D, s0);
                } else {
                    const double lo = dpp_double_from_lower_lane(d[NS - 1], NEG_INF_D);  // state lane*NS - 1
                    asg_frame_sum<NS>(col, gs, ga, d, e, lo);
                }
            }
        } else {
            // off the recursion's chain, for the whole chunk at once (independent of each other, so they overlap): the
            // emission factors P_f(j) = exp(e_f(j) - m_f) in [0, 1] with m_f the frame's largest emission (0 for a frame of
            // -inf alone, whose every P is 0), 0 on the lanes beyond k; the m_f go straight into log Z.  (Rows at and past nf
            // repeat the segment's last frame: computed, never used.)
            double P[ALIGN_CH];
#pragma unroll
            for (int f = 0; f < ALIGN_CH; ++f) {
                const float ef = on ? em[f * 64 + lane] : -INFINITY;
                const float mx = wave_max_f(ef);
                const double m = mx == -INFINITY ? 0.0 : (double)mx;
                P[f] = exp((double)ef - m);
                msum += f < nf ? m : 0.0;
            }
#pragma unroll
            for (int f = 0; f < ALIGN_CH; ++f) {
                if (f >= nf) continue;  // (wave-uniform)
                if (f == 0 && t0 == 0) {
                    v = sj * P[0];
                    continue;
                }
                // the previous frame's values through LDS.  Only this wave touches vec and a wave's LDS operations complete in
                // order, so the fences are of wavefront scope: they keep the compiler from moving the accesses and wait for
                // nothing (a work-group fence would wait for the next chunk's loads from HBM, every chunk)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                vec[lane] = v;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // k multiply-adds on four chains.  The values come back as broadcast reads, 32 of them in flight at once (two
                // per instruction: vec is 16-byte aligned), so a frame pays the LDS latency once and not once per grapheme;
                // past k they are the zeros of the lanes that own no grapheme, against zero columns.  Beside the sums, the
                // largest of the values read (they are >= 0, so the order of their high words is theirs): every lane reads
                // the same ones and finds the same exponent.
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                int top = 0;
#pragma unroll
                for (int h0 = 0; h0 < KR; h0 += 32) {
                    if (h0 >= k) continue;  // (wave-uniform)
                    double x[32];
#pragma unroll
                    for (int u = 0; u < 32; ++u) x[u] = vec[h0 + u];
#pragma unroll
                    for (int u = 0; u < 32; u += 4) {
                        a0 = fma(x[u], gcol[h0 + u], a0);
                        a1 = fma(x[u + 1], gcol[h0 + u + 1], a1);
                        a2 = fma(x[u + 2], gcol[h0 + u + 2], a2);
                        a3 = fma(x[u + 3], gcol[h0 + u + 3], a3);
                        top = max(max(top, __double2hiint(x[u])),
                                  max(max(__double2hiint(x[u + 1]), __double2hiint(x[u + 2])), __double2hiint(x[u + 3])));
                    }
                }
                // rescale by the power of two that puts the PREVIOUS frame's largest value into [1, 2): exact, known without
                // a reduction, and one frame changes a value by a factor in [e^-(|g| + |e|), k e^|g|], far inside a double.
                // Whatever exponent is taken is the one that is counted, so log Z stays exact; all zeros stay zeros.
                const int ex = ((top >> 20) & 0x7ff) - 1023;
                v = ldexp(((a0 + a1) + (a2 + a3)) * P[f], -ex);
                esum += ex;
            }
        }
    }

    if (wave == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (lane * NS + j == L - 1) fin[0] = d[j];
    } else {
        // log Z = log(sum_j v(j)) + the exponents taken out + the emission maxima: ONE reduction and one log per segment; a
        // sum of 0 (a frame without emissions, closed tables) gives -inf
        const double logz = log(wave_sum_d(v)) + (double)esum * LN2_D + msum;
        if (lane == 0) fin[1] = logz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double N = fin[0], Z = fin[1];
        *res = (N == NEG_INF_D || Z == NEG_INF_D) ? -INFINITY : (float)(N * LN2_D - Z);
    }
}

int states_per_lane(int seg_l_max) { return seg_l_max <= 64 ? 1 : (seg_l_max <= 128 ? 2 : (seg_l_max <= 256 ? 4 : 8)); }

template <int NS, int KR>
int launch_segment(const float* logq, const float* trans, const float* init, const int32_t* labels, const int32_t* input_len,
                   const int32_t* segments, float* out, int batch, int t_out, int k, int l_max, int n_segments, int seg_l_max,
                   hipStream_t s) {
    hipLaunchKernelGGL((asg_segment_kernel<NS, KR>), dim3(n_segments), dim3(128), segment_lds_bytes(k), s, logq, trans, init, labels,
                       input_len, segments, out, batch, t_out, k, l_max, seg_l_max);
    return sl_check_launch("sl_asg_segment_scores");
}

}  // namespace

extern "C" size_t sl_asg_segment_scores_workspace_bytes(int n_segments, int seg_l_max, int k) {
    (void)n_segments;
    (void)seg_l_max;
    (void)k;
    return 0;  // a segment's lattices live in its work-group's registers and LDS
}

extern "C" int sl_asg_segment_scores(const float* logq, const float* trans, const float* init, const int32_t* labels,
                                     const int32_t* input_len, const int32_t* segments, float* log_posterior, int batch,
                                     int t_out, int k, int l_max, int n_segments, int seg_l_max, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    if (k < 2 || k > 64) {
        sl_set_error("sl_asg_segment_scores: k = %d outside 2 <= k <= 64 (one lane per grapheme)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (seg_l_max < 0 || seg_l_max > SEG_L_LIMIT) {
        sl_set_error("sl_asg_segment_scores: seg_l_max = %d outside 0 <= seg_l_max <= %d (at most 8 states per lane)", seg_l_max,
                     SEG_L_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    if (n_segments < 1) {
        sl_set_error("sl_asg_segment_scores: n_segments = %d, need n_segments >= 1", n_segments);
        return SL_ERR_UNSUPPORTED;
    }
    SL_CHECK_ARG(batch > 0 && t_out > 0 && l_max >= 0, "sl_asg_segment_scores: need batch, t_out > 0 and l_max >= 0");
    SL_CHECK_ARG(logq, "sl_asg_segment_scores: logq is a null pointer");
    SL_CHECK_ARG(trans, "sl_asg_segment_scores: trans is a null pointer");
    SL_CHECK_ARG(init, "sl_asg_segment_scores: init is a null pointer");
    SL_CHECK_ARG(labels || l_max == 0, "sl_asg_segment_scores: labels is a null pointer (l_max = %d)", l_max);
    SL_CHECK_ARG(input_len, "sl_asg_segment_scores: input_len is a null pointer");
    SL_CHECK_ARG(segments, "sl_asg_segment_scores: segments is a null pointer");
    SL_CHECK_ARG(log_posterior, "sl_asg_segment_scores: log_posterior is a null pointer");
    const size_t need = sl_asg_segment_scores_workspace_bytes(n_segments, seg_l_max, k);
    if (workspace_bytes < need || (need > 0 && workspace == nullptr)) {
        sl_set_error("sl_asg_segment_scores: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
#define SL_SEGMENT(NS_)                                                                                                      \
    return k <= 32 ? launch_segment<NS_, 32>(logq, trans, init, labels, input_len, segments, log_posterior, batch, t_out, k, l_max, \
                                             n_segments, seg_l_max, s)                                                         \
                   : launch_segment<NS_, 64>(logq, trans, init, labels, input_len, segments, log_posterior, batch, t_out, k, l_max, \
                                             n_segments, seg_l_max, s)
    switch (states_per_lane(seg_l_max)) {
        case 1: SL_SEGMENT(1);
        case 2: SL_SEGMENT(2);
        case 4: SL_SEGMENT(4);
        default: SL_SEGMENT(8);
    }
#undef SL_SEGMENT
}
