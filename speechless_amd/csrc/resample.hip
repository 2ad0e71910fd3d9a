// resample.hip -- sample-rate conversion of a ragged batch of utterances on the GPU ("Resampling").
//
// Replaces the host resampler the reference reaches through librosa.load(file, sr=16000) (speechless/labeled_example.py:200-205):
// a band-limited (Kaiser-windowed sinc) interpolator, restated as a polyphase FIR bank by speechless_amd/resample.py:
//
//      y[t] = sum_{j < width} h[r][j] * x[n - (left - 1) + j],    n = (t p) div q,  r = (t p) mod q,   x = 0 outside the utterance
//
// The weights depend on t only through r, and r repeats with period q.  A work-group takes a tile of RS_TILE consecutive
// outputs of one utterance and lays it out as rows of S = k q columns (the smallest multiple of q that is >= 256): the thread
// of column c owns the outputs T0 + c + m S, m < ceil(RS_TILE / S) <= RS_ROWS (the kernel is instantiated per row count, so no
// accumulator is carried for a row the tile does not have).  They share ONE bank row (r is the same, n advances by k p per row),
// so a weight is read once for up to eight FMAs.  The tile's input span is staged in LDS once (zeros outside the utterance:
// the inner loop has no bounds test); the bank goes through LDS in chunks of a few taps of every row, read from L2 with
// coalesced loads -- per-lane row walks in global memory would hold one cache line per lane and overrun the 32 KB L1.
// n and r come from one 64-bit division per tile and one 32-bit division per thread.
#include "common.h"

namespace {

constexpr int RS_TILE = SL_RESAMPLE_TILE;  // outputs per work-group tile
constexpr int RS_ROWS = 8;                 // most accumulators per thread: RS_TILE / 256
constexpr int RS_CHUNK_FLOATS = 4096;      // bank chunk in LDS: q * taps-per-chunk <= this
constexpr int RS_LDS_BYTES = 64 * 1024;
constexpr int RS_LOADS = 8;                // bank loads a thread keeps in flight

static_assert(RS_ROWS * 256 == RS_TILE, "a tile is RS_ROWS rows of at least 256 columns");

template <int ROWS>  // rows of the tile: ceil(RS_TILE / cols)
__global__ __launch_bounds__(1024) void resample_polyphase_kernel(const float* __restrict__ audio, const long* __restrict__ in_offsets,
                                                                   const int* __restrict__ in_lengths, float* __restrict__ out,
                                                                   const long* __restrict__ out_offsets,
                                                                   const float* __restrict__ bank, int p, int q, int left, int width,
                                                                   int cols, int span, int chunk, int lpr_log2) {
    extern __shared__ float rs_lds[];
    float* xs = rs_lds;          // span floats: x[n0 - (left - 1) + i]
    float* hs = rs_lds + span;   // q rows of `chunk` taps, row stride chunk | 1
    const int hs_stride = chunk | 1;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int b = blockIdx.y;
    const int len = in_lengths[b];
    if (len <= 0) return;  // (uniform over the work-group)
    const long n_res = (long)len * q / p;                  // outputs the filter produces
    const long n_out = ((long)len * q + p - 1) / p;        // ... and what is written: at most one zero behind them
    const long n_tiles = (n_out + RS_TILE - 1) / RS_TILE;
    const float* x = audio + in_offsets[b];
    float* y = out + out_offsets[b];
    const int row_step = cols / q * p;  // input samples between two rows of a column
    const int load_row0 = tid >> lpr_log2, load_lane = tid & ((1 << lpr_log2) - 1), load_rows = nthreads >> lpr_log2;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long t0 = tile * RS_TILE;
        const long a0 = t0 * p;
        const long n0 = a0 / q;
        const int r0 = (int)(a0 - n0 * q);
        __syncthreads();  // the previous tile's readers of xs are done
        const long g0 = n0 - (left - 1);
        for (int i = tid; i < span; i += nthreads) {
            const long g = g0 + i;
            xs[i] = (g >= 0 && g < len) ? x[g] : 0.f;
        }
        const bool active = tid < cols;
        const int a = r0 + (active ? tid : 0) * p;  // < q + 1023 p, and the LDS limit keeps p below 8 q <= 8192
        const int dn = a / q, r = a - dn * q;
        int xo[ROWS];
        bool live[ROWS];
#pragma unroll
        for (int m = 0; m < ROWS; ++m) {
            live[m] = active && tid + m * cols < RS_TILE;  // (a dead row reads row 0's samples: always inside xs)
            xo[m] = dn + (live[m] ? m * row_step : 0);
        }
        float acc[ROWS];
#pragma unroll
        for (int m = 0; m < ROWS; ++m) acc[m] = 0.f;
        for (int j0 = 0; j0 < width; j0 += chunk) {
            const int jc = min(chunk, width - j0);
            __syncthreads();  // xs is staged (first pass); the previous chunk has been read
            // 2^lpr_log2 lanes walk the taps of a row, the thread's other bits pick the row: no division
            // (RS_LOADS rows at a time, all loads in flight before the first LDS write: one L2 round trip per batch, not per row)
            if (load_row0 < load_rows)
                for (int jj = load_lane; jj < jc; jj += 1 << lpr_log2)
                    for (int row = load_row0; row < q; row += RS_LOADS * load_rows) {
                        float v[RS_LOADS];
#pragma unroll
                        for (int u = 0; u < RS_LOADS; ++u) {
                            const int rr = row + u * load_rows;
                            v[u] = rr < q ? bank[(long)rr * width + j0 + jj] : 0.f;
                        }
#pragma unroll
                        for (int u = 0; u < RS_LOADS; ++u) {
                            const int rr = row + u * load_rows;
                            if (rr < q) hs[rr * hs_stride + jj] = v[u];
                        }
                    }
            __syncthreads();
            if (active) {
                const float* hrow = hs + r * hs_stride;
                const float* xp = xs + j0;
#pragma unroll 4
                for (int jj = 0; jj < jc; ++jj) {
                    const float h = hrow[jj];
#pragma unroll
                    for (int m = 0; m < ROWS; ++m) acc[m] = fmaf(h, xp[xo[m] + jj], acc[m]);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < ROWS; ++m) {
            const long t = t0 + tid + m * cols;
            if (live[m] && t < n_out) y[t] = t < n_res ? acc[m] : 0.f;
        }
    }
}

int gcd_int(int a, int b) {
    while (b) {
        const int c = a % b;
        a = b;
        b = c;
    }
    return a;
}

}  // namespace

extern "C" int sl_resample_polyphase(const float* audio, const int64_t* in_offsets, const int32_t* in_lengths, float* out,
                                     const int64_t* out_offsets, const float* bank, int batch, int p, int q, int left, int width,
                                     void* stream) {
    SL_CHECK_ARG(audio && in_offsets && in_lengths && out && out_offsets && bank, "sl_resample_polyphase: null pointer");
    SL_CHECK_ARG(batch > 0 && batch <= 65535, "sl_resample_polyphase: batch = %d must lie in [1, 65535]", batch);
    SL_CHECK_ARG(p >= 1 && q >= 1, "sl_resample_polyphase: p = %d and q = %d must be positive", p, q);
    SL_CHECK_ARG(p != q, "sl_resample_polyphase: p == q = %d (equal rates: there is nothing to convert)", p);
    SL_CHECK_ARG(gcd_int(p, q) == 1, "sl_resample_polyphase: p = %d and q = %d must be in lowest terms", p, q);
    SL_CHECK_ARG(left >= 1 && left <= width, "sl_resample_polyphase: left = %d must lie in [1, width = %d]", left, width);
    if (q > SL_RESAMPLE_MAX_PHASES || width > SL_RESAMPLE_MAX_TAPS) {
        sl_set_error("sl_resample_polyphase: a bank of %d phases x %d taps is over the limits (%d phases, %d taps)", q, width,
                     SL_RESAMPLE_MAX_PHASES, SL_RESAMPLE_MAX_TAPS);
        return SL_ERR_UNSUPPORTED;
    }
    const int cols = q >= 256 ? q : (256 + q - 1) / q * q;  // columns of a tile: a multiple of q in [256, 1024]
    const int threads = (cols + 63) / 64 * 64;
    const int64_t span = (int64_t)(RS_TILE - 1) * p / q + 1 + width;  // input samples under one tile
    const int chunk = width < RS_CHUNK_FLOATS / q ? width : RS_CHUNK_FLOATS / q;
    const int64_t lds = (span + (int64_t)q * (chunk | 1)) * (int64_t)sizeof(float);
    if (lds > RS_LDS_BYTES) {
        sl_set_error("sl_resample_polyphase: a tile of %d outputs at p / q = %d / %d spans %lld input samples: %lld bytes of LDS, "
                     "the limit is %d", RS_TILE, p, q, (long long)span, (long long)lds, RS_LDS_BYTES);
        return SL_ERR_UNSUPPORTED;
    }
    // lengths live in HBM: the grid is fixed and every work-group strides over its utterance's tiles
    int per_utt = (4096 + batch - 1) / batch;
    if (per_utt > 2048) per_utt = 2048;
    int lpr_log2 = 0;  // lanes that walk one bank row of a chunk: the power of two above the chunk's taps, 256 at most
    while ((1 << lpr_log2) < chunk && lpr_log2 < 8) ++lpr_log2;
    const int rows = (RS_TILE + cols - 1) / cols;  // 2 .. RS_ROWS
#define RS_LAUNCH(R)                                                                                                            \
    hipLaunchKernelGGL(resample_polyphase_kernel<R>, dim3(per_utt, batch), dim3(threads), (size_t)lds, (hipStream_t)stream,     \
                       audio, (const long*)in_offsets, in_lengths, out, (const long*)out_offsets, bank, p, q, left, width, cols, \
                       (int)span, chunk, lpr_log2)
    switch (rows) {
        case 2: RS_LAUNCH(2); break;
        case 3: RS_LAUNCH(3); break;
        case 4: RS_LAUNCH(4); break;
        case 5: RS_LAUNCH(5); break;
        case 6: RS_LAUNCH(6); break;
        case 7: RS_LAUNCH(7); break;
        default: RS_LAUNCH(8); break;
    }
#undef RS_LAUNCH
    return sl_check_launch("sl_resample_polyphase");
}
