// ctc_align.hip -- CTC forced alignment (Viterbi over the CTC lattice + backtrace) for gfx950.
//
// No reference counterpart: the reference only CONSUMES word timings (speechless/labeled_example.py:32-60, PositionalLabel,
// and :219-234, LabeledExampleFromFile.sections()).  This produces them from a net's output distribution and a transcript.
// Semantics (bit for bit, fp32): include/speechless_hip.h, sl_ctc_align.
//
// Kernel ctc_align_kernel<NJ, BP_LDS>: ONE WAVE per utterance, NJ consecutive lattice states per lane in registers (lane l
// holds states l*NJ .. l*NJ + NJ - 1; NJ = 4 / 8 / 16 for S = 2L+1 <= 256 / 512 / 1024, as ctc_grad_kernel<NJ, ...> picks
// by l_max).  Per frame: the highest state of the lane below arrives by one DPP wave_shr:1 move (a lane's first state
// is a blank, which never skips), every state takes max(stay, s-1, s-2) with the tie rule and adds its emission (one
// exact max chain + ONE rounded add: no FMA can form -- ctc_frame of lattice.h, which ctc_align_long.hip runs too), and the 2-bit
// backpointers of the lane's NJ states -- one byte / short / dword -- are stored as one row of 16*NJ bytes per frame in which
// state s sits at bits 2s.  Emissions come from LDS: the wave stages ALIGN_CH frames of logq rows (k <= 64 floats, one coalesced
// read per frame) while it works on the previous ALIGN_CH frames (EmissionStager of lattice.h).
//   BP_LDS = 1: the T' rows fit the work-group's LDS (config 3: 500 frames x 128 bytes) and the backtrace reads them there.
//   BP_LDS = 0: rows go to the workspace in HBM; the backtrace copies windows of BT_W frames (the whole rows: contiguous
//   bytes) into LDS, the next window's loads in flight while the current one is resolved, so that no frame of the T'-long
//   backtrace waits on a dependent HBM load.
// The backtrace is run by every lane of the wave on the same (wave-uniform) state: its LDS reads are broadcasts, and lane
// t - w0 keeps the state of frame t, so the path leaves as one coalesced store per window.
#include "lattice.h"

namespace {

template <int NJ>
struct BpWord;
template <>
struct BpWord<4> { typedef uint8_t T; };
template <>
struct BpWord<8> { typedef uint16_t T; };
template <>
struct BpWord<16> { typedef uint32_t T; };

__host__ __device__ constexpr int row_bytes(int nj) { return 16 * nj; }  // 64 lanes x 2 bits x nj states

// LDS: [logq chunk ALIGN_CH x 64 floats][final scores 64*NJ floats][backpointer rows: T' rows (BP_LDS) or two windows of BT_W rows]
template <int NJ, bool BP_LDS>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ logq, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ label_len,
                                                        const int32_t* __restrict__ input_len, int32_t* __restrict__ path,
                                                        float* __restrict__ score, uint8_t* __restrict__ bp_hbm, int t_out,
                                                        int k, int l_max) {
    typedef typename BpWord<NJ>::T Word;
    constexpr int R = row_bytes(NJ);
    extern __shared__ float smem[];
    float* em = smem;
    float* fin = em + ALIGN_CH * 64;
    uint8_t* rows = (uint8_t*)(fin + 64 * NJ);

    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int blank = k - 1;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    const int S = 2 * L + 1;
    const int32_t* lab = labels + (long)b * l_max;
    int32_t* prow = path + (long)b * t_out;

    // feasibility: T >= L + (adjacent equal labels)
    int reps = 0;
    for (int i0 = 1; i0 < L; i0 += 64) {
        const int i = i0 + lane;
        const bool eq = i < L && lab[i] == lab[i - 1];
        reps += __popcll(__ballot(eq));
    }
    for (int t = T + lane; t < t_out; t += 64) prow[t] = -1;
    if (T < L + reps || T == 0) {
        for (int t = lane; t < T; t += 64) prow[t] = -1;
        if (lane == 0) score[b] = (T == 0 && L == 0) ? 0.f : -INFINITY;
        return;
    }

    // per-lane lattice: lane l holds states l*NJ .. l*NJ + NJ - 1, at the virtual frame -1 (lattice.h)
    int col[NJ / 2];
    bool skip[NJ / 2];
    float d[NJ];
    ctc_states_init<NJ>(col, skip, lab, lane * NJ, S, k);
    // delta of a virtual frame -1: state 0 at 0, the rest at -inf, so that frame 0 yields delta_0(0) = logq_0(blank) and
    // delta_0(1) = logq_0(l_0) exactly (0 + x == x) and every other state -inf
#pragma unroll
    for (int j = 0; j < NJ; ++j) d[j] = lane * NJ + j == 0 ? 0.f : -INFINITY;

    const float* lq = logq + (long)b * t_out * k;
    EmissionStager<64> stg;
    stg.prefetch(lq, 0, T, k, 0, lane);
    Word* bp_lds = (Word*)rows + lane;
    Word* bp_g = (Word*)(bp_hbm + (long)b * t_out * R) + lane;
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
            const float lo1 = dpp_float_from_lower_lane(d[NJ - 1], -INFINITY);
            const uint32_t word = ctc_frame<NJ>(col, skip, d, e, e[blank], lo1);
            const int t = t0 + f;
            if (BP_LDS)
                bp_lds[(long)t * (R / sizeof(Word))] = (Word)word;
            else
                bp_g[(long)t * (R / sizeof(Word))] = (Word)word;
        }
    }

    // end state: the better of S-1 and S-2, S-1 on a tie
#pragma unroll
    for (int j = 0; j < NJ; ++j) fin[lane * NJ + j] = d[j];
    __syncthreads();
    int s = S - 1;
    if (S >= 2 && fin[S - 2] > fin[S - 1]) s = S - 2;
    if (lane == 0) score[b] = fin[s];

    // backtrace, windows [w0, w0 + BT_W) from the last one down
    const int nwin = (T + BT_W - 1) / BT_W;
    constexpr int V = BT_W * R / 16 / 64;  // u32x4 per lane of one window
    constexpr int VR = BP_LDS ? 1 : V;  // (no window registers when the rows stay in LDS)
    u32x4 wreg[VR];
    const uint8_t* bp_utt = bp_hbm + (long)b * t_out * R;
    if (!BP_LDS) {
        load_window<u32x4, VR, R>(wreg, bp_utt, nwin - 1, T, lane);
        store_window<u32x4, VR, R>(wreg, rows, nwin - 1, lane);
    }
    for (int w = nwin - 1; w >= 0; --w) {
        const int w0 = w * BT_W;
        const int w1 = T - w0 < BT_W ? T : w0 + BT_W;
        if (!BP_LDS && w > 0) load_window<u32x4, VR, R>(wreg, bp_utt, w - 1, T, lane);
        __syncthreads();
        const uint8_t* base = BP_LDS ? rows + (long)w0 * R : rows + (w & 1) * BT_W * R;
        int mine = -1;
        for (int t = w1 - 1; t >= w0; --t) {
            if (lane == t - w0) mine = s;
            if (t > 0) {
                const uint32_t byte = base[(t - w0) * R + (s >> 2)];
                s -= (byte >> (2 * (s & 3))) & 3u;
            }
        }
        if (w0 + lane < w1) prow[w0 + lane] = mine;
        if (!BP_LDS && w > 0) {
            __syncthreads();
            store_window<u32x4, VR, R>(wreg, rows, w - 1, lane);
        }
    }
}

template <int NJ, bool BP_LDS>
size_t align_lds_bytes(int t_out) {
    return (size_t)(ALIGN_CH * 64 + 64 * NJ) * sizeof(float) + (size_t)(BP_LDS ? t_out : 2 * BT_W) * row_bytes(NJ);
}

int states_per_lane(int l_max) { return 2 * l_max + 1 <= 256 ? 4 : (2 * l_max + 1 <= 512 ? 8 : 16); }

bool bp_in_lds(int nj, int t_out) {
    switch (nj) {
        case 4: return align_lds_bytes<4, true>(t_out) <= (size_t)ALIGN_LDS_MAX;
        case 8: return align_lds_bytes<8, true>(t_out) <= (size_t)ALIGN_LDS_MAX;
        default: return align_lds_bytes<16, true>(t_out) <= (size_t)ALIGN_LDS_MAX;
    }
}

template <int NJ, bool BP_LDS>
int launch_align(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len, int32_t* path,
                 float* score, void* workspace, int batch, int t_out, int k, int l_max, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)ctc_align_kernel<NJ, BP_LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   ALIGN_LDS_MAX);
        attr_set = true;
    }
    const size_t lds = align_lds_bytes<NJ, BP_LDS>(t_out);
    hipLaunchKernelGGL((ctc_align_kernel<NJ, BP_LDS>), dim3(batch), dim3(64), lds, s, logq,
                       labels, label_len, input_len, path, score, (uint8_t*)workspace, t_out, k, l_max);
    return sl_check_launch("sl_ctc_align");
}

}  // namespace

extern "C" size_t sl_ctc_align_workspace_bytes(int batch, int t_out, int l_max) {
    if (batch <= 0 || t_out <= 0 || l_max < 0 || l_max > 511) return 0;
    const int nj = states_per_lane(l_max);
    return bp_in_lds(nj, t_out) ? 0 : (size_t)batch * t_out * row_bytes(nj);
}

extern "C" int sl_ctc_align(const float* logq, const int32_t* labels, const int32_t* label_len, const int32_t* input_len,
                            int32_t* path, float* score, int batch, int t_out, int k, int l_max, void* workspace,
                            size_t workspace_bytes, void* stream) {
    SL_CHECK_ARG(batch > 0 && t_out > 0 && l_max >= 0, "sl_ctc_align: need batch, t_out > 0 and l_max >= 0");
    SL_CHECK_ARG(logq && label_len && input_len && path && score && (labels || l_max == 0), "sl_ctc_align: null pointer");
    if (k <= 1 || k > 64) {
        sl_set_error("sl_ctc_align: k = %d outside 1 < k <= 64 (one lane per class)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (l_max > 511) {
        sl_set_error("sl_ctc_align: label length %d > 511 unsupported (at most 1023 lattice states)", l_max);
        return SL_ERR_UNSUPPORTED;
    }
    const size_t need = sl_ctc_align_workspace_bytes(batch, t_out, l_max);
    if (workspace_bytes < need || (need > 0 && workspace == nullptr)) {
        sl_set_error("sl_ctc_align: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    const hipStream_t s = (hipStream_t)stream;
    const int nj = states_per_lane(l_max);
    const bool lds = need == 0;
#define SL_ALIGN(NJ_)                                                                                                      \
    return lds ? launch_align<NJ_, true>(logq, labels, label_len, input_len, path, score, workspace, batch, t_out, k, l_max, s) \
               : launch_align<NJ_, false>(logq, labels, label_len, input_len, path, score, workspace, batch, t_out, k, l_max, s)
    if (nj == 4) SL_ALIGN(4);
    if (nj == 8) SL_ALIGN(8);
    SL_ALIGN(16);
#undef SL_ALIGN
}
