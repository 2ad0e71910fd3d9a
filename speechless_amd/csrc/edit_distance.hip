// edit_distance.hip -- letter and word error counts (Levenshtein distance, unit costs) of a batch of index rows, for gfx950.
//
// Stands in for the two `editdistance.eval` calls of the reference's result object (speechless/net.py:31-37: over the
// characters of expected / predicted, and over their .split()), which this project restates on the host as
// speechless_amd.net.edit_distance.  Semantics: include/speechless_hip.h, sl_edit_distance.  Integer arithmetic only: exact.
//
// Kernel edit_distance_kernel<NJ>: ONE WORK-GROUP OF TWO WAVES per utterance.  Both rows are staged in LDS once; wave 0
// tokenises `a` and wave 1 `b` into word spans (start, end) by a ballot over the separator predicate -- a word's number is
// the count of word starts below it --, then wave 0 runs the letter distance while wave 1 runs the word distance: the two
// dependent chains of an utterance overlap, and B utterances occupy B compute units.
//
// The distance itself (wave_levenshtein<NJ>) walks the rows of the DP matrix, one row per symbol of `b`, with the columns
// (symbols of `a`) spread over the wave: lane l keeps columns l*NJ+1 .. l*NJ+NJ of the previous row in registers (NJ = 1 /
// 4 / 16 for a_max <= 64 / 256 / 1024).  Within a row
//   cur[j] = min(t[j], cur[j-1] + 1),  t[j] = min(prev[j] + 1, prev[j-1] + (a[j] != b[r]))
// and the horizontal dependency is a prefix minimum: cur[j] - j = min over k <= j of (t[k] - k) (with t[0] = r, column 0).
// So a row costs one wave_shr:1 move (prev[j-1] of a lane's first column), NJ local steps and ONE wave-wide prefix-min
// (four row_shr steps, row_bcast:15, row_bcast:31): no lane ever waits on a 64-long chain.  The symbol of `b` is a wave-
// uniform LDS read (a broadcast).  For the word pass a "symbol" is a span; two spans are equal iff they have the same length
// and the same indices, compared in place in the staged rows with an early exit (no hashing: nothing to confirm).
//
// Per-lane state is 2*NJ..3*NJ registers indexed by unrolled constants: no scratch (build.py NO_SCRATCH).
#include "common.h"

namespace {

constexpr int BIG = 0x3fffffff;
constexpr int A_MAX = 1024;          // 64 lanes x NJ = 16 columns
constexpr int LDS_LIMIT = 64 * 1024;  // static + dynamic LDS a kernel gets without an attribute

__host__ __device__ constexpr int span_slots(int n) { return (n + 1) / 2; }  // most words a row of n indices can hold
// LDS ints: a row, b row, a word starts / ends, b word starts / ends, the two word counts
__host__ __device__ constexpr long lds_ints(int a_max, int b_max) {
    return (long)a_max + b_max + 2L * span_slots(a_max) + 2L * span_slots(b_max) + 2;
}

__device__ __forceinline__ int dpp_from_lower_lane(int v, int lane0_value) {  // lane l <- lane l-1 (wave_shr:1)
    return __builtin_amdgcn_update_dpp(lane0_value, v, 0x138, 0xf, 0xf, false);
}

// inclusive prefix minimum over the 64 lanes of the wave
__device__ __forceinline__ int wave_prefix_min(int x) {
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x111, 0xf, 0xf, false));  // row_shr:1
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x112, 0xf, 0xf, false));  // row_shr:2
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x114, 0xf, 0xf, false));  // row_shr:4
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x118, 0xf, 0xf, false));  // row_shr:8
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    x = min(x, __builtin_amdgcn_update_dpp(BIG, x, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return x;
}

// symbols of the letter pass: the indices themselves
struct Letters {
    const int* a_row;
    const int* b_row;
    typedef int Key;
    __device__ __forceinline__ Key a(int i) const { return a_row[i]; }
    __device__ __forceinline__ Key b(int i) const { return b_row[i]; }
    __device__ __forceinline__ static Key none() { return 0; }
    __device__ __forceinline__ bool differ(Key x, Key y) const { return x != y; }
};

// symbols of the word pass: spans [start, start + len) of the staged rows
struct Words {
    const int* a_row;
    const int* b_row;
    const int* a_start;
    const int* a_end;
    const int* b_start;
    const int* b_end;
    struct Key {
        int start, len;
    };
    __device__ __forceinline__ Key a(int i) const { return Key{a_start[i], a_end[i] - a_start[i]}; }
    __device__ __forceinline__ Key b(int i) const { return Key{b_start[i], b_end[i] - b_start[i]}; }
    __device__ __forceinline__ static Key none() { return Key{0, -1}; }  // (no word has length -1: never equal)
    __device__ __forceinline__ bool differ(Key x, Key y) const {
        if (x.len != y.len) return true;
        for (int i = 0; i < x.len; ++i)
            if (a_row[x.start + i] != b_row[y.start + i]) return true;
        return false;
    }
};

// Levenshtein distance between la symbols of `a` (la <= 64 * NJ) and lb symbols of `b`, by one full wave; the lane that
// holds the last column stores the result.
template <int NJ, class Sym>
__device__ __forceinline__ void wave_levenshtein(const Sym sym, int la, int lb, int lane, int32_t* out) {
    typename Sym::Key ka[NJ];
    int prev[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane * NJ + j;  // column c + 1 holds symbol c of a
        ka[j] = c < la ? sym.a(c) : Sym::none();
        prev[j] = c + 1;              // row 0
    }
    for (int r = 0; r < lb; ++r) {  // row r + 1
        const typename Sym::Key kb = sym.b(r);
        int diag = dpp_from_lower_lane(prev[NJ - 1], r);  // (column 0 of row r holds r)
        int m = BIG;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int t = min(prev[j] + 1, diag + (sym.differ(ka[j], kb) ? 1 : 0));
            diag = prev[j];
            m = min(m, t - (lane * NJ + j + 1));
            prev[j] = m;  // prefix minimum of t[k] - k over this lane's columns
        }
        const int below = min(dpp_from_lower_lane(wave_prefix_min(m), BIG), r + 1);  // ... over every column to the left
#pragma unroll
        for (int j = 0; j < NJ; ++j) prev[j] = min(prev[j], below) + (lane * NJ + j + 1);
    }
    if (la == 0) {
        if (lane == 0) *out = lb;
        return;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (lane * NJ + j + 1 == la) *out = prev[j];
}

// word spans of row[0 .. n): a word is a maximal run of indices != space (space < 0: the whole row).  Returns their number.
__device__ __forceinline__ int wave_tokenise(const int* row, int n, int space, int lane, int* start, int* end) {
    int started = 0, ended = 0;  // the k-th end closes the k-th start, whichever chunk either lies in
    for (int p0 = 0; p0 < n; p0 += 64) {
        const int p = p0 + lane;
        const bool in_word = p < n && (space < 0 || row[p] != space);
        const bool after_word = in_word && p > 0 && (space < 0 || row[p - 1] != space);
        const bool before_word = in_word && p + 1 < n && (space < 0 || row[p + 1] != space);
        const bool is_start = in_word && !after_word;
        const bool is_end = in_word && !before_word;
        const unsigned long long starts = __ballot(is_start);
        const unsigned long long ends = __ballot(is_end);
        const unsigned long long lower = (1ull << lane) - 1ull;
        if (is_start) start[started + __popcll(starts & lower)] = p;
        if (is_end) end[ended + __popcll(ends & lower)] = p + 1;
        started += __popcll(starts);
        ended += __popcll(ends);
    }
    return started;
}

// LDS: [a row a_max][b row b_max][a starts][a ends][b starts][b ends][words of a, words of b]
template <int NJ>
__global__ __launch_bounds__(128) void edit_distance_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ a_len,
                                                             long a_stride, const int32_t* __restrict__ b,
                                                             const int32_t* __restrict__ b_len, long b_stride, int a_max,
                                                             int b_max, int space, int32_t* __restrict__ letter_errors,
                                                             int32_t* __restrict__ word_errors,
                                                             int32_t* __restrict__ a_word_count) {
    extern __shared__ int smem[];
    int* a_row = smem;
    int* b_row = a_row + a_max;
    int* a_start = b_row + b_max;
    int* a_end = a_start + span_slots(a_max);
    int* b_start = a_end + span_slots(a_max);
    int* b_end = b_start + span_slots(b_max);
    int* counts = b_end + span_slots(b_max);

    const int u = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int la = a_len[u];
    const int lb = b_len[u];
    if (la < 0 || la > a_max || lb < 0 || lb > b_max) {  // the whole work-group leaves: nothing of the rows is read
        if (tid == 0) {
            letter_errors[u] = -1;
            word_errors[u] = -1;
            if (a_word_count) a_word_count[u] = -1;
        }
        return;
    }
    const int32_t* ga = a + u * a_stride;
    const int32_t* gb = b + u * b_stride;
    for (int p = tid; p < la; p += 128) a_row[p] = ga[p];
    for (int p = tid; p < lb; p += 128) b_row[p] = gb[p];
    __syncthreads();
    if (wave == 0) {
        const int n = wave_tokenise(a_row, la, space, lane, a_start, a_end);
        if (lane == 0) counts[0] = n;
    } else {
        const int n = wave_tokenise(b_row, lb, space, lane, b_start, b_end);
        if (lane == 0) counts[1] = n;
    }
    __syncthreads();
    if (wave == 0) {
        wave_levenshtein<NJ>(Letters{a_row, b_row}, la, lb, lane, letter_errors + u);
    } else {
        const int wa = counts[0], wb = counts[1];
        if (lane == 0 && a_word_count) a_word_count[u] = wa;
        wave_levenshtein<NJ>(Words{a_row, b_row, a_start, a_end, b_start, b_end}, wa, wb, lane, word_errors + u);
    }
}

template <int NJ>
int launch(const int32_t* a, const int32_t* a_len, int a_stride, const int32_t* b, const int32_t* b_len, int b_stride,
           int batch, int a_max, int b_max, int space, int32_t* letter_errors, int32_t* word_errors, int32_t* a_word_count,
           hipStream_t s) {
    const size_t lds = (size_t)lds_ints(a_max, b_max) * sizeof(int);
    SL_LAUNCH_MAIN((edit_distance_kernel<NJ>), dim3(batch), dim3(128), lds, s, a, a_len, (long)a_stride, b, b_len,
                   (long)b_stride, a_max, b_max, space, letter_errors, word_errors, a_word_count);
    return sl_check_launch("sl_edit_distance");
}

}  // namespace

extern "C" int sl_edit_distance_supported(int a_max, int b_max) {
    return a_max >= 0 && b_max >= 0 && a_max <= A_MAX && lds_ints(a_max, b_max) * (long)sizeof(int) <= LDS_LIMIT;
}

extern "C" int sl_edit_distance(const int32_t* a, const int32_t* a_len, int a_stride, const int32_t* b, const int32_t* b_len,
                                int b_stride, int batch, int a_max, int b_max, int space, int32_t* letter_errors,
                                int32_t* word_errors, int32_t* a_word_count, void* stream) {
    SL_CHECK_ARG(batch > 0 && a_max >= 0 && b_max >= 0, "sl_edit_distance: need batch > 0 and a_max, b_max >= 0");
    SL_CHECK_ARG(a_len && b_len && letter_errors && word_errors && (a || a_max == 0) && (b || b_max == 0),
                 "sl_edit_distance: null pointer");
    SL_CHECK_ARG(a_max <= a_stride && b_max <= b_stride,
                 "sl_edit_distance: a_max = %d / b_max = %d above the row stride %d / %d", a_max, b_max, a_stride, b_stride);
    if (!sl_edit_distance_supported(a_max, b_max)) {
        sl_set_error("sl_edit_distance: a_max = %d, b_max = %d unsupported (a_max <= %d, and both rows with their word spans "
                     "in %d bytes of LDS: sl_edit_distance_supported)", a_max, b_max, A_MAX, LDS_LIMIT);
        return SL_ERR_UNSUPPORTED;
    }
    const hipStream_t s = (hipStream_t)stream;
#define SL_ED(NJ_) \
    return launch<NJ_>(a, a_len, a_stride, b, b_len, b_stride, batch, a_max, b_max, space, letter_errors, word_errors, a_word_count, s)
    if (a_max <= 64) SL_ED(1);
    if (a_max <= 256) SL_ED(4);
    SL_ED(16);
#undef SL_ED
}
