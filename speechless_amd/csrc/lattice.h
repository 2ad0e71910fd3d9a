// lattice.h -- what the lattice kernels that keep their states in registers share (ctc_align.hip, ctc_align_long.hip, asg.hip,
// asg_align.hip, asg_align_long.hip, ctc_segment.hip, asg_segment.hip, ctc_spot.hip):
//   - the clamps of lengths and labels, and the neighbour-lane move;
//   - the windows of whole backpointer rows that a one-wave backtrace pulls from HBM into LDS (load_window / store_window),
//     and the bands of them that a long aligner's backtrace pulls (load_band / store_band);
//   - for the four forced aligners, each piece that include/speechless_hip.h defines bit for bit, ONCE: the CTC states of a
//     thread and their frame step (ctc_states_init / ctc_frame), the ASG ones (asg_states_init / asg_frame), and the stager of
//     their emissions (EmissionStager, ALIGN_CH);
//   - for the segment posteriors (ctc_segment.hip, asg_segment.hip), the SUMMING frame steps over the same states
//     (ctc_frame_sum, asg_frame_sum), in doubles;
//   - for the phrase search (ctc_spot.hip), the frame step that carries a begin-frame tag with every score (ctc_spot_frame).
// No helper here holds a barrier, a fence or a return: those stay in the kernels, next to the argument for their uniformity.
#pragma once
#include "common.h"
#include "lse_double.h"

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

__device__ __forceinline__ int dpp_int_from_lower_lane(int v, int lane0_value) {  // the same move of an integer
    return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ double dpp_double_from_lower_lane(double v, double lane0_value) {  // the same move, both halves
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(lane0_value), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(lane0_value), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
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

// ---------------------------------------------------------------------------------------------- the forced aligners
constexpr int ALIGN_CH = 16;  // frames of logq per LDS staging chunk
constexpr int ALIGN_LDS_MAX = 160 * 1024;

// Emission stager of a work-group of NT threads (64: one wave, whose wave index is the constant 0).  A chunk is ALIGN_CH rows of
// 64 floats in LDS, row f the logq row of frame t + f (clamped to frame T - 1: never read) with the columns >= k at 0.  Round m
// of the work-group moves rows m * NT/64 .. m * NT/64 + NT/64 - 1, a wave one row and a lane one class of it; a thread holds its
// values in pre[] while they are in flight.  CTC chunks start at frame 0, ASG chunks at frame 1.
// (A struct, while the states below are functions over arrays of the kernel's own.  Neither form is a matter of taste: they
// are the ones under which this compiler allocates registers as it did for the hand-inlined loops -- pre[] behind an array
// reference becomes one 16-register tuple, the states as struct members are split into scalars and re-paired.  Nothing in the
// build guards that (NO_SCRATCH of build.py catches spills only): after a change here or a new compiler, compare the VGPR
// counts with the table of DESIGN.md 3.2 and re-time with the tools named there.)
template <int NT>
struct EmissionStager {
    static constexpr int PRE = ALIGN_CH * 64 / NT;  // staged logq values per thread and chunk
    static_assert(NT % 64 == 0 && ALIGN_CH * 64 % NT == 0, "a chunk is staged by whole rounds of the work-group");
    float pre[PRE];

    __device__ __forceinline__ void prefetch(const float* lq, int t, int T, int k, int wave, int lane) {
#pragma unroll
        for (int m = 0; m < PRE; ++m) {
            const int r = m * (NT / 64) + wave;
            // (the row outside the select: inside it k is known positive, and the 64-bit product costs three scalar
            // instructions more per row -- 3 % of a chunk of the one-wave kernels)
            const float* row = lq + (long)(t + r < T ? t + r : T - 1) * k;
            pre[m] = lane < k ? row[lane] : 0.f;
        }
    }
    __device__ __forceinline__ void store(float* em, int wave, int lane) const {
#pragma unroll
        for (int m = 0; m < PRE; ++m) em[(m * (NT / 64) + wave) * 64 + lane] = pre[m];
    }
};

// NJ consecutive states of the CTC lattice of a label (even: blank, odd 2p + 1: letter p), the first of them even: col[] the
// label columns of the odd states, skip[] whether they may be entered from s-2, d[] the scores.
// ctc_states_init gathers col[] and skip[]; the kernel itself puts d[] at the virtual frame -1 (as the ASG kernels put theirs at
// frame 0): with the scores first written inside a helper the compiler schedules the frame step differently, measurably slower
// (DESIGN.md 3.2).
template <int NJ>
__device__ __forceinline__ void ctc_states_init(int (&col)[NJ / 2], bool (&skip)[NJ / 2], const int32_t* lab,
                                                int first_state, int S, int k) {
#pragma unroll
    for (int q = 0; q < NJ / 2; ++q) {
        const int s = first_state + 2 * q + 1;
        const int pos = (s - 1) >> 1;
        int c = k - 1;
        bool sk = false;
        if (s < S) {
            c = clamp_label(lab[pos], k);
            sk = pos >= 1 && lab[pos - 1] != lab[pos];
        }
        col[q] = c;
        skip[q] = sk;
    }
}
// One frame: e its staged logq row, eb = e[blank], lo1 the state below the first (s-1 of the first state, which is even and never
// skips, and s-2 of the second).  max(stay, s-1, s-2) by strict >, so the earlier candidate wins a tie, then ONE rounded add.
// Returns the 2-bit backpointers (0 stay, 1 from s-1, 2 from s-2), state j at bits 2j.
template <int NJ>
__device__ __forceinline__ uint32_t ctc_frame(const int (&col)[NJ / 2], const bool (&skip)[NJ / 2], float (&d)[NJ], const float* e,
                                              float eb, float lo1) {
    uint32_t word = 0;
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {  // descending: d[j-1], d[j-2] still hold frame t-1
        const float p1 = j >= 1 ? d[j - 1] : lo1;
        float best = d[j];
        uint32_t bp = 0;
        if (p1 > best) {
            best = p1;
            bp = 1;
        }
        if (j & 1) {
            const float p2 = j >= 2 ? d[j - 2] : lo1;
            if (skip[j >> 1] && p2 > best) {
                best = p2;
                bp = 2;
            }
            d[j] = best + e[col[j >> 1]];
        } else {
            d[j] = best + eb;
        }
        word |= bp << (2 * j);
    }
    return word;
}
// The same frame with a begin-frame TAG in place of the backpointer, for the phrase search of sl_ctc_spot (ctc_spot.hip): g[] the
// tag of each score, lo1g the tag of lo1.  The winning candidate's tag travels with its score (one compare-select more per
// candidate), and a state that ends the frame at -inf has tag -1.  The same strict > in the same order, then ONE rounded add.
template <int NJ>
__device__ __forceinline__ void ctc_spot_frame(const int (&col)[NJ / 2], const bool (&skip)[NJ / 2], float (&d)[NJ], int (&g)[NJ],
                                               const float* e, float eb, float lo1, int lo1g) {
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {  // descending: d[j-1], d[j-2] and their tags still hold frame t-1
        const float p1 = j >= 1 ? d[j - 1] : lo1;
        const int g1 = j >= 1 ? g[j - 1] : lo1g;
        float best = d[j];
        int tag = g[j];
        if (p1 > best) {
            best = p1;
            tag = g1;
        }
        if (j & 1) {
            const float p2 = j >= 2 ? d[j - 2] : lo1;
            const int g2 = j >= 2 ? g[j - 2] : lo1g;
            if (skip[j >> 1] && p2 > best) {
                best = p2;
                tag = g2;
            }
            best += e[col[j >> 1]];
        } else {
            best += eb;
        }
        d[j] = best;
        g[j] = best == -INFINITY ? -1 : tag;
    }
}
// The same frame with the SUM in place of the max, for the forward (alpha) lattice of sl_ctc_segment_scores: d[] in doubles and
// log2 units, a(s) = log2(2^a(s) + 2^a(s-1) [+ 2^a(s-2) where the state may be entered from s-2]) + logq(label(s)) * log2(e),
// the sum by lse2_long / lse3_long of lse_double.h (the step of ctc_long.hip) and the emission by one fma.  No backpointers.
// A state beyond the label has the blank's column and nothing above it reads it.
template <int NJ>
__device__ __forceinline__ void ctc_frame_sum(const int (&col)[NJ / 2], const bool (&skip)[NJ / 2], double (&d)[NJ], const float* e,
                                              float eb, double lo1) {
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j) {  // descending: d[j-1], d[j-2] still hold frame t-1
        const double p1 = j >= 1 ? d[j - 1] : lo1;
        if (j & 1) {
            const double p2 = j >= 2 ? d[j - 2] : lo1;
            d[j] = fma((double)e[col[j >> 1]], LOG2E_D, lse3_long(d[j], p1, skip[j >> 1] ? p2 : NEG_INF_D));
        } else {
            d[j] = fma((double)eb, LOG2E_D, lse2_long(d[j], p1));
        }
    }
}

// NS consecutive states of a label under the ASG criterion (state s: letter s of the label): col[] the emission column, gs[]
// the stay score g(l_s, l_s), ga[] the score g(l_{s-1}, l_s) of the move into the state, d[] the scores.
// asg_states_init gathers col[], gs[] and ga[]; the kernel itself puts d[] at frame 0 (state 0 open, the rest at -inf), for
// the reason given at ctc_states_init: written by a helper, asg_align_long_kernel<16> takes 114 VGPRs instead of 89.  A state
// beyond the label stays at -inf for good (-inf + 0, and a move that adds -inf)
template <int NS>
__device__ __forceinline__ void asg_states_init(int (&col)[NS], float (&gs)[NS], float (&ga)[NS],
                                                const int32_t* lab, int first_state, int L, int k, const float* trans) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int s = first_state + j;
        col[j] = 0;
        gs[j] = 0.f;
        ga[j] = -INFINITY;
        if (s < L) {
            const int c = clamp_label(lab[s], k);
            col[j] = c;
            gs[j] = trans[c * k + c];
            if (s > 0) ga[j] = trans[clamp_label(lab[s - 1], k) * k + c];
        }
    }
}
// One frame: e its staged logq row, lo the state below the first.  stay = d(s) + g(l_s, l_s), move = d(s-1) + g(l_{s-1}, l_s),
// the larger (stay on a tie) plus the emission: three separately rounded adds and no multiply.  word[j]: the wave's lanes whose
// state j moved.
template <int NS>
__device__ __forceinline__ void asg_frame(const int (&col)[NS], const float (&gs)[NS], const float (&ga)[NS], float (&d)[NS],
                                          const float* e, float lo, uint64_t (&word)[NS]) {
#pragma unroll
    for (int j = NS - 1; j >= 0; --j) {  // descending: d[j-1] still holds frame t-1
        const float stay = d[j] + gs[j];
        const float move = (j >= 1 ? d[j - 1] : lo) + ga[j];
        const bool mv = move > stay;
        word[j] = __ballot(mv);
        d[j] = (mv ? move : stay) + e[col[j]];
    }
}
// The same frame with the SUM in place of the max, for the numerator (alpha) lattice of sl_asg_segment_scores: d[] in doubles
// and log2 units, gs[] / ga[] the same scores in doubles times log2(e); a(s) = log2(2^(a(s) + gs) + 2^(a(s-1) + ga)) + e(l_s) *
// log2(e), the sum by lse2_long of lse_double.h and the emission by one fma.  No backpointers.  A state beyond the label
// stays at -inf as above.
template <int NS>
__device__ __forceinline__ void asg_frame_sum(const int (&col)[NS], const double (&gs)[NS], const double (&ga)[NS], double (&d)[NS],
                                              const float* e, double lo) {
#pragma unroll
    for (int j = NS - 1; j >= 0; --j) {  // descending: d[j-1] still holds frame t-1
        const double stay = d[j] + gs[j];
        const double move = (j >= 1 ? d[j - 1] : lo) + ga[j];
        d[j] = fma((double)e[col[j]], LOG2E_D, lse2_long(stay, move));
    }
}
// Band of a long aligner's backtrace window w: rows w*BT_W .. min(T, w*BT_W + BT_W) - 1, dwords base .. base + BAND - 1 of each
// (row_dw dwords per row), into registers; and from there into an LDS window of BT_W x BAND dwords
template <int BAND>
__device__ __forceinline__ void load_band(uint32_t (&wreg)[BAND], const uint32_t* bp_utt, int row_dw, int w, int T, int base,
                                          int lane) {
    const int w0 = w * BT_W;
    const int rows = T - w0 < BT_W ? T - w0 : BT_W;
#pragma unroll
    for (int m = 0; m < BAND; ++m) {
        const int i = m * 64 + lane;  // i = row * BAND + c
        const int row = i / BAND;
        const int c = i - row * BAND;
        wreg[m] = (row < rows && base + c < row_dw) ? bp_utt[(long)(w0 + row) * row_dw + base + c] : 0u;
    }
}
template <int BAND>
__device__ __forceinline__ void store_band(const uint32_t (&wreg)[BAND], uint32_t* win, int lane) {
#pragma unroll
    for (int m = 0; m < BAND; ++m) win[m * 64 + lane] = wreg[m];
}
