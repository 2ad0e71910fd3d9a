// ctc_spot.hip -- CTC phrase search for gfx950: where in an utterance (or an hour-long recording) a phrase is said, and how well.
// A Viterbi search over the phrase's CTC states in which every frame may open a new occurrence at no cost, with a begin-frame
// tag that travels with every score: no backpointers, no backtrace.  The non-overlapping best occurrences are picked on the
// device in the same launch.
//
// No reference counterpart.  Semantics: include/speechless_hip.h, sl_ctc_spot (defined bit for bit).
//
// Kernel ctc_spot_kernel<NJ>: ONE WAVE per query in a work-group of 64 threads, NJ consecutive lattice states per lane in
// registers (NJ = 2 / 4 / 8 / 16 for q_max <= 63 / 127 / 255 / 511, the split of ctc_segment.hip).  The lattice is the aligners'
// (lattice.h: ctc_states_init, the neighbour-lane move, EmissionStager) one state up: lattice state 0 -- the aligners' leading
// blank -- is the FILLER, which lane 0 puts back to score 0 and tag t before every frame, lattice state s + 1 is the header's state
// s, and the header's last state 2L - 2 is lattice state 2L - 1, the last letter.  The trailing blank is computed and never read.
// The frame step is ctc_spot_frame: ctc_frame with the tag's compare-select in place of the backpointer bits.
// Per chunk of ALIGN_CH frames the lane that owns the last letter leaves its score and tag in LDS and 16 lanes write them to the
// workspace (and to frame_score / frame_begin) in one row each.  The picking then runs over the workspace: per hit one pass of
// the wave that suppresses what the previous hit overlaps and takes the arg-max of the rest.
#include "lattice.h"

namespace {

constexpr int SPOT_Q_LIMIT = 511;
constexpr int SPOT_HITS_LIMIT = 64;

// the better of two (score, frame) candidates of the picking: the larger score, on equal scores the smaller frame
__device__ __forceinline__ void spot_better(float& s, int& t, float s2, int t2) {
    if (s2 > s || (s2 == s && t2 < t)) {
        s = s2;
        t = t2;
    }
}

template <int NJ>
__global__ __launch_bounds__(64) void ctc_spot_kernel(const float* __restrict__ logq, const int32_t* __restrict__ input_len,
                                                       const int32_t* __restrict__ queries, const int32_t* __restrict__ query_len,
                                                       const int32_t* __restrict__ query_utt, const float* __restrict__ min_score,
                                                       int32_t* __restrict__ hits, float* __restrict__ hit_score,
                                                       int32_t* __restrict__ n_hits, float* __restrict__ frame_score,
                                                       int32_t* __restrict__ frame_begin, float* __restrict__ ws_score,
                                                       int32_t* __restrict__ ws_begin, int batch, int t_out, int k, int q_max,
                                                       int max_hits) {
    __shared__ float em[ALIGN_CH * 64];
    __shared__ float fs[ALIGN_CH];  // the last letter's score and tag at the frames of a chunk
    __shared__ int fb[ALIGN_CH];

    const int lane = threadIdx.x;
    const long q = blockIdx.x;
    float* wsc = ws_score + q * t_out;
    int32_t* wbg = ws_begin + q * t_out;
    float* fsc = frame_score ? frame_score + q * t_out : nullptr;
    int32_t* fbg = frame_begin ? frame_begin + q * t_out : nullptr;
    const int32_t* lab = queries + q * q_max;

    // (b, L and T are uniform over the wave, and so is every branch on them)
    const int b = query_utt[q];
    int L = query_len[q];
    L = L < 0 ? 0 : (L > q_max ? q_max : L);
    int T = 0;
    if (b >= 0 && b < batch && L > 0) {
        T = input_len[b];
        T = T < 0 ? 0 : (T > t_out ? t_out : T);
    }

    if (T > 0) {
        const int S = 2 * L;  // lattice states 0 (filler) .. 2L - 1 (last letter)
        const int blank = k - 1;
        const int own_lane = (S - 1) / NJ;
        const int own_j = (S - 1) % NJ;  // odd

        int col[NJ / 2];
        bool skip[NJ / 2];
        float d[NJ];
        int g[NJ];
        ctc_states_init<NJ>(col, skip, lab, lane * NJ, S, k);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            d[j] = -INFINITY;
            g[j] = -1;
        }

        const float* lq = logq + (long)b * t_out * k;
        EmissionStager<64> stg;
        stg.prefetch(lq, 0, T, k, 0, lane);
        for (int t0 = 0; t0 < T; t0 += ALIGN_CH) {
            __syncthreads();  // (the chunk before has been read: em by the frames, fs / fb by the row writers)
            stg.store(em, 0, lane);
            __syncthreads();
            if (t0 + ALIGN_CH < T) stg.prefetch(lq, t0 + ALIGN_CH, T, k, 0, lane);
            const int nf = T - t0 < ALIGN_CH ? T - t0 : ALIGN_CH;
#pragma unroll
            for (int f = 0; f < ALIGN_CH; ++f) {
                if (f >= nf) continue;  // (wave-uniform; a break keeps the loop from unrolling)
                const float* e = em + f * 64;
                if (lane == 0) {  // the filler: score 0 at every frame, and whoever leaves it begins at this frame
                    d[0] = 0.f;
                    g[0] = t0 + f;
                }
                const float lo1 = dpp_float_from_lower_lane(d[NJ - 1], -INFINITY);
                const int lo1g = dpp_int_from_lower_lane(g[NJ - 1], -1);
                ctc_spot_frame<NJ>(col, skip, d, g, e, e[blank], lo1, lo1g);
                float sv = d[1];
                int gv = g[1];
#pragma unroll
                for (int j = 3; j < NJ; j += 2) {
                    if (own_j == j) {
                        sv = d[j];
                        gv = g[j];
                    }
                }
                if (lane == own_lane) {
                    fs[f] = sv;
                    fb[f] = gv;
                }
            }
            __syncthreads();
            if (lane < nf) {
                const float sv = fs[lane];
                const int gv = fb[lane];
                wsc[t0 + lane] = sv;
                wbg[t0 + lane] = gv;
                if (fsc) fsc[t0 + lane] = sv;
                if (fbg) fbg[t0 + lane] = gv;
            }
        }
    }
    for (int t = T + lane; t < t_out; t += 64) {
        if (fsc) fsc[t] = -INFINITY;
        if (fbg) fbg[t] = -1;
    }
    // the rows of the workspace were written by other lanes than read them below
    __syncthreads();

    // ---- hit picking: pass h suppresses what hit h-1 overlaps and takes the arg-max of what is left.  A lane reads and
    // writes the same frames of the workspace in every pass, in program order.
    const float thr = min_score[q];
    int32_t* hq = hits + q * max_hits * 2;
    float* hs = hit_score + q * max_hits;
    int n = 0;
    int pb = 0, pe = -1;  // the previous hit's frames [pb, pe]; none yet
    for (; n < max_hits; ++n) {
        float best = -INFINITY;
        int bt = 0x7fffffff;
        for (int u = lane; u < T; u += 64) {
            float s = wsc[u];
            if (pe >= 0 && u >= pb && wbg[u] <= pe) {
                s = -INFINITY;
                wsc[u] = s;
            }
            if (s > -INFINITY && s >= thr && s > best) {  // (ascending u: the lane's smallest frame of its best score)
                best = s;
                bt = u;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) spot_better(best, bt, __shfl_xor(best, m, 64), __shfl_xor(bt, m, 64));
        if (!(best > -INFINITY)) break;  // (uniform: every lane holds the wave's best)
        pe = bt;
        pb = wbg[bt];
        if (lane == 0) {
            hq[2 * n] = pb;
            hq[2 * n + 1] = bt + 1;
            hs[n] = best;
        }
    }
    if (lane >= n && lane < max_hits) {
        hq[2 * lane] = -1;
        hq[2 * lane + 1] = -1;
        hs[lane] = -INFINITY;
    }
    if (lane == 0) n_hits[q] = n;
}

int states_per_lane(int q_max) { return q_max <= 63 ? 2 : (q_max <= 127 ? 4 : (q_max <= 255 ? 8 : 16)); }

}  // namespace

extern "C" size_t sl_ctc_spot_workspace_bytes(int n_queries, int t_out, int q_max) {
    if (n_queries < 1 || t_out < 1 || q_max < 1 || q_max > SPOT_Q_LIMIT) return 0;
    return (size_t)n_queries * (size_t)t_out * (sizeof(float) + sizeof(int32_t));  // every query's per-frame score and begin
}

extern "C" int sl_ctc_spot(const float* logq, const int32_t* input_len, const int32_t* queries, const int32_t* query_len,
                           const int32_t* query_utt, const float* min_score, int32_t* hits, float* hit_score, int32_t* n_hits,
                           float* frame_score, int32_t* frame_begin, int batch, int t_out, int k, int n_queries, int q_max,
                           int max_hits, void* workspace, size_t workspace_bytes, void* stream) {
    if (k <= 1 || k > 64) {
        sl_set_error("sl_ctc_spot: k = %d outside 1 < k <= 64 (one lane per class)", k);
        return SL_ERR_UNSUPPORTED;
    }
    if (q_max < 1 || q_max > SPOT_Q_LIMIT) {
        sl_set_error("sl_ctc_spot: q_max = %d outside 1 <= q_max <= %d (at most 1023 lattice states per query)", q_max,
                     SPOT_Q_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    if (max_hits < 1 || max_hits > SPOT_HITS_LIMIT) {
        sl_set_error("sl_ctc_spot: max_hits = %d outside 1 <= max_hits <= %d (one lane per hit slot)", max_hits, SPOT_HITS_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    if (n_queries < 1) {
        sl_set_error("sl_ctc_spot: n_queries = %d, need n_queries >= 1", n_queries);
        return SL_ERR_UNSUPPORTED;
    }
    SL_CHECK_ARG(batch > 0 && t_out > 0, "sl_ctc_spot: need batch, t_out > 0");
    SL_CHECK_ARG(logq, "sl_ctc_spot: logq is a null pointer");
    SL_CHECK_ARG(input_len, "sl_ctc_spot: input_len is a null pointer");
    SL_CHECK_ARG(queries, "sl_ctc_spot: queries is a null pointer");
    SL_CHECK_ARG(query_len, "sl_ctc_spot: query_len is a null pointer");
    SL_CHECK_ARG(query_utt, "sl_ctc_spot: query_utt is a null pointer");
    SL_CHECK_ARG(min_score, "sl_ctc_spot: min_score is a null pointer");
    SL_CHECK_ARG(hits, "sl_ctc_spot: hits is a null pointer");
    SL_CHECK_ARG(hit_score, "sl_ctc_spot: hit_score is a null pointer");
    SL_CHECK_ARG(n_hits, "sl_ctc_spot: n_hits is a null pointer");
    const size_t need = sl_ctc_spot_workspace_bytes(n_queries, t_out, q_max);
    if (workspace_bytes < need || workspace == nullptr) {
        sl_set_error("sl_ctc_spot: workspace too small (%zu < %zu)", workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    float* ws_score = (float*)workspace;
    int32_t* ws_begin = (int32_t*)(ws_score + (size_t)n_queries * (size_t)t_out);
    const hipStream_t s = (hipStream_t)stream;
#define SL_SPOT(NJ_)                                                                                                          \
    hipLaunchKernelGGL((ctc_spot_kernel<NJ_>), dim3(n_queries), dim3(64), 0, s, logq, input_len, queries, query_len, query_utt, \
                       min_score, hits, hit_score, n_hits, frame_score, frame_begin, ws_score, ws_begin, batch, t_out, k, q_max, \
                       max_hits);                                                                                             \
    break
    switch (states_per_lane(q_max)) {
        case 2: SL_SPOT(2);
        case 4: SL_SPOT(4);
        case 8: SL_SPOT(8);
        default: SL_SPOT(16);
    }
#undef SL_SPOT
    return sl_check_launch("sl_ctc_spot");
}
