// optimizer.hip -- the parameter update: Keras-2.0 Adam and the five rules beside it, flat or fused with the operand repack,
// with or without gradient clipping; the squared gradient norm and the clip factor.  ONE element update (opt_element<RULE>),
// one flat kernel, one fused kernel -- and on the host one launcher for each (launch_flat, launch_fused) that every entry
// point goes through.
#include "common.h"

namespace {

// ONE definition of the element update for every Adam kernel of this file, with the contraction pinned: left to the
// compiler, `b1 * m + (1 - b1) * g` becomes fma(b1, m, (1 - b1) * g) in one kernel and fma(1 - b1, g, b1 * m) in another,
// and the plain elementwise kernel (the sharded optimizer's) would differ from the fused Adam + repack kernel in the
// last bit -- data-parallel runs with and without the sharded optimizer are held to bit-identical weights.
__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, const float lr_t, const float b1,
                                             const float b2, const float eps) {
#pragma clang fp contract(off)
    const float gm = (1.f - b1) * g;
    const float gv = (1.f - b2) * g * g;
    m = __builtin_fmaf(b1, m, gm);
    v = __builtin_fmaf(b2, v, gv);
    const float step = lr_t * m / (sqrtf(v) + eps);
    p = p - step;
}

// Gradient clipping (sl_*_clipped): what the update sees in place of g.  Comparisons, not fminf / fmaxf: a NaN gradient stays
// a NaN, as through Keras' clip.  gs == 1 and cv == 0 leave g's bits alone.
__device__ __forceinline__ float clipped_grad(const float g, const float gs, const float cv) {
    const float s = g * gs;
    if (cv > 0.f) return s > cv ? cv : (s < -cv ? -cv : s);
    return s;
}

// The other Keras-2.0 rules (include/speechless_hip.h "Keras-2.0 optimizers beside Adam"), each ONE definition with the
// contraction pinned like adam_element: the flat kernel (unfused step, sharded slices, ASG tables) and the fused update +
// repack kernel must give the same bits.  lr is the decayed rate (Adamax: already divided by 1 - b1^t, on the host).
__device__ __forceinline__ void sgd_element(float& p, const float g, float& m, const float lr, const float momentum,
                                            const float nesterov) {
#pragma clang fp contract(off)
    const float lg = lr * g;
    const float v = __builtin_fmaf(momentum, m, -lg);
    m = v;
    p = nesterov != 0.f ? p + __builtin_fmaf(momentum, v, -lg) : p + v;
}

__device__ __forceinline__ void rmsprop_element(float& p, const float g, float& a, const float lr, const float rho,
                                                const float eps) {
#pragma clang fp contract(off)
    const float gg = (1.f - rho) * g * g;
    a = __builtin_fmaf(rho, a, gg);
    const float step = lr * g / (sqrtf(a) + eps);
    p = p - step;
}

__device__ __forceinline__ void adagrad_element(float& p, const float g, float& a, const float lr, const float eps) {
#pragma clang fp contract(off)
    a = __builtin_fmaf(g, g, a);
    const float step = lr * g / (sqrtf(a) + eps);
    p = p - step;
}

__device__ __forceinline__ void adadelta_element(float& p, const float g, float& a, float& d, const float lr, const float rho,
                                                 const float eps) {
#pragma clang fp contract(off)
    const float gg = (1.f - rho) * g * g;
    a = __builtin_fmaf(rho, a, gg);
    const float u = g * sqrtf(d + eps) / sqrtf(a + eps);
    const float step = lr * u;
    p = p - step;
    const float uu = (1.f - rho) * u * u;
    d = __builtin_fmaf(rho, d, uu);
}

// (comparisons, not fmaxf: a NaN gradient stays a NaN in u, as through Keras' maximum)
__device__ __forceinline__ void adamax_element(float& p, const float g, float& m, float& u, const float lr_t, const float b1,
                                               const float b2, const float eps) {
#pragma clang fp contract(off)
    const float gm = (1.f - b1) * g;
    m = __builtin_fmaf(b1, m, gm);
    const float bu = b2 * u, ag = fabsf(g);
    u = bu > ag ? bu : ag;
    const float step = lr_t * m / (u + eps);
    p = p - step;
}

// RULE: an SL_OPT_* id.  Every update kernel below is an instantiation over it; the four coefficients travel as
// (lr, c0, c1, eps) -- Adam: lr_t, b1, b2; SGD: lr, momentum, nesterov (0 / 1); RMSprop, Adadelta: lr, rho; Adagrad: lr;
// Adamax: lr_t, b1, b2.  A rule with one state slot never touches s1 (the kernels get NULL for it).
__host__ __device__ constexpr bool opt_two_slots(int rule) {
    return rule == SL_OPT_ADAM || rule == SL_OPT_ADADELTA || rule == SL_OPT_ADAMAX;
}
template <int RULE>
__device__ __forceinline__ void opt_element(float& p, const float g, float& s0, float& s1, const float lr, const float c0,
                                            const float c1, const float eps) {
    if (RULE == SL_OPT_ADAM) adam_element(p, g, s0, s1, lr, c0, c1, eps);
    if (RULE == SL_OPT_SGD) sgd_element(p, g, s0, lr, c0, c1);
    if (RULE == SL_OPT_RMSPROP) rmsprop_element(p, g, s0, lr, c0, eps);
    if (RULE == SL_OPT_ADAGRAD) adagrad_element(p, g, s0, lr, eps);
    if (RULE == SL_OPT_ADADELTA) adadelta_element(p, g, s0, s1, lr, c0, eps);
    if (RULE == SL_OPT_ADAMAX) adamax_element(p, g, s0, s1, lr, c0, c1, eps);
}

// CLIP: the gradient goes through clipped_grad first (*gscale read once per thread: NULL = 1); CLIP = false is the kernel
// as it was -- a launch with no clipping asked for goes to that instantiation
template <bool CLIP = false, int RULE = SL_OPT_ADAM>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long n4, float lr_t, float b1, float b2, float eps,
                            const float* __restrict__ gscale = nullptr, float cv = 0.f) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 gv = ((const f32x4*)g)[i];
    if (CLIP) {
        const float gs = gscale ? *gscale : 1.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = clipped_grad(gv[j], gs, cv);
    }
    constexpr bool TWO = opt_two_slots(RULE);
    f32x4 mv = ((f32x4*)m)[i];
    f32x4 vv = TWO ? ((f32x4*)v)[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 pv = ((f32x4*)p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        opt_element<RULE>(pj, gv[j], mj, vj, lr_t, b1, b2, eps);
        pv[j] = pj, mv[j] = mj, vv[j] = vj;
    }
    ((f32x4*)m)[i] = mv;
    if (TWO) ((f32x4*)v)[i] = vv;
    ((f32x4*)p)[i] = pv;
}

// Fused Adam + operand repack: a single pass over a layer's fp32 master weights / gradient / moments [k][cin][cout] (+ the
// bias block that follows them) that also emits both device operand layouts
//   w_fwd [cout][k][cin]   (tile transposed through LDS)   and   w_dgrad[cin][k-1-tap][cout]
// 4 fp32 reads + 3 fp32 writes + 2 narrow writes per parameter instead of Adam (4r+3w) followed by pack (1r+2w).
// The unit of work is a TILE: 64 input channels x ADAM_CO_T output channels of one tap, so that a w_fwd run is 64 input
// channels (a whole 128-byte line of a bf16 operand) and the fp32 runs are ADAM_CO_T * 4 bytes.  cin_pad is only a multiple of
// 32 and cout_pad only of 64: the last tile of a row / column is cut (AdamTile::rows / cols), its spare lanes load the tile's
// first vector again and store nothing.  After a layer's k * nci * nco weight tiles come its nco bias tiles (one row).
// PLANES = 3 (bf16x3, T = unsigned short): the operand rows are [w_hi | w_hi | w_lo], w_hi = bf16(w), w_lo = bf16(w - w_hi).
// FMT (PLANES = 3 only): 0 = bf16 planes, 1 = fp16 planes of wscale * w (f16x3: wscale a power of two, see split3.hip)
template <int FMT>
__device__ __forceinline__ u32x2 pack_hi4(float a0, float a1, float a2, float a3) {
    if (FMT == 1) return (u32x2){pack_f16x2(a0, a1), pack_f16x2(a2, a3)};
    return (u32x2){pack_bf16x2(a0, a1), pack_bf16x2(a2, a3)};
}
template <int FMT>
__device__ __forceinline__ u32x2 pack_lo4(float a0, float a1, float a2, float a3) {
    if (FMT == 1) {
        auto lo = [](float v) { return v - f16_bits_to_f32(f32_to_f16_bits(v)); };
        return (u32x2){pack_f16x2(lo(a0), lo(a1)), pack_f16x2(lo(a2), lo(a3))};
    }
    auto lo = [](float v) { return v - bf16_bits_to_f32(f32_to_bf16_bits(v)); };
    return (u32x2){pack_bf16x2(lo(a0), lo(a1)), pack_bf16x2(lo(a2), lo(a3))};
}
constexpr int ADAM_CI_T = 64;                 // input channels of a tile: one w_fwd run
constexpr int ADAM_CO_T = 128;                // output channels of a tile: 512-byte fp32 runs, 256-byte w_dgrad runs
constexpr int ADAM_NV = ADAM_CO_T / 4;        // 16-byte vectors in a tile row
constexpr int ADAM_RPP = 256 / ADAM_NV;       // tile rows one pass of the 256 threads covers
constexpr int ADAM_N = ADAM_CI_T / ADAM_RPP;  // passes = 16-byte loads per thread and stream
constexpr int ADAM_TN = ADAM_CO_T / 16;       // passes of the transposed store (16 threads per 64-channel run)

// p, g, m and v are read once and written once per step, with nothing for a cache to keep: nontemporal.  The operand copies,
// which the next forward reads, keep the default policy.  (profiles/adam_copy_bw_ab.json: the larger of the two gains)
__device__ __forceinline__ f32x4 stream_load4(const float* a) { return __builtin_nontemporal_load((const f32x4*)a); }
__device__ __forceinline__ void stream_store4(float* a, const f32x4 x) { __builtin_nontemporal_store(x, (f32x4*)a); }

// every trainable layer in ONE launch: the small layers' updates (0.46 M parameters each, 8 us per launch of pure
// latency) ride along with the big ones.  blockIdx.x is a tile id through all layers; the table maps it to its layer.
struct AdamTable {
    int n;
    int tile_begin[SL_ADAM_MAX_LAYERS + 1];
    long offset[SL_ADAM_MAX_LAYERS];  // first weight of the layer in the flat fp32 buffers
    void* wf[SL_ADAM_MAX_LAYERS];
    void* wd[SL_ADAM_MAX_LAYERS];
    int k[SL_ADAM_MAX_LAYERS], cin[SL_ADAM_MAX_LAYERS], cout[SL_ADAM_MAX_LAYERS];
};

// one tile, the same in every thread of the work-group
struct AdamTile {
    int k, cin, cout;
    int tap;         // == k: a bias tile (one row of `cols` floats behind the weights, no operand copy)
    int ci0, co0;    // the tile's first input / output channel
    int rows, cols;  // what of the 64 x ADAM_CO_T tile the layer has: 32 or 64 rows (bias: 1); a multiple of 64 columns
    long base;       // the tile's first element in the flat fp32 buffers
    void *wf, *wd;
};

__device__ __forceinline__ AdamTile adam_tile(const AdamTable& t, const int id) {
    int layer = 0;
    while (layer + 1 < t.n && id >= t.tile_begin[layer + 1]) ++layer;
    AdamTile tl;
    tl.k = t.k[layer], tl.cin = t.cin[layer], tl.cout = t.cout[layer];
    tl.wf = t.wf[layer], tl.wd = t.wd[layer];
    const int nco = (tl.cout + ADAM_CO_T - 1) / ADAM_CO_T, nci = (tl.cin + ADAM_CI_T - 1) / ADAM_CI_T;
    const int local = id - t.tile_begin[layer];  // co tile fastest, then ci tile, then tap; the nco bias tiles last (tap == k)
    const int rest = local / nco;
    tl.co0 = (local - rest * nco) * ADAM_CO_T;
    tl.tap = rest / nci;
    tl.ci0 = (rest - tl.tap * nci) * ADAM_CI_T;
    tl.rows = tl.tap == tl.k ? 1 : min(ADAM_CI_T, tl.cin - tl.ci0);
    tl.cols = min(ADAM_CO_T, tl.cout - tl.co0);
    tl.base = t.offset[layer] + ((long)tl.tap * tl.cin + tl.ci0) * tl.cout + tl.co0;  // (bias: k * cin * cout + co0)
    return tl;
}

// One tile: all of its loads first (ADAM_N 16-byte vectors per thread and stream), then the update, the fp32 stores and both
// operand copies.  thread -> (row ty + n * ADAM_RPP, vector tx) of the tile.
template <typename T, bool ADAM = true, int PLANES = 1, int FMT = 0, bool CLIP = false, int RULE = SL_OPT_ADAM>
__device__ __forceinline__ void adam_pack_tile(float (&lds)[ADAM_CI_T][ADAM_CO_T + 1], const AdamTile& tl,
                                               float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, float lr_t, float b1, float b2, float eps, float wscale,
                                               float gs, float cv) {
    constexpr bool TWO = opt_two_slots(RULE);  // (a one-slot rule: v is NULL, neither read nor written)
    const bool bias = tl.tap == tl.k;
    const int tx = threadIdx.x % ADAM_NV, ty = threadIdx.x / ADAM_NV;
    // a lane outside a cut tile takes the tile's first vector (a valid address, a line its neighbours load anyway), so that the
    // loads stay unconditional; it stores nothing.  (both are computed again behind the loads: kept in registers they cost the third work-group per CU)
    auto in_tile = [&](int n) { return n * ADAM_RPP + ty < tl.rows && tx * 4 < tl.cols; };
    auto index_of = [&](int n) { return tl.base + (in_tile(n) ? (long)(n * ADAM_RPP + ty) * tl.cout + tx * 4 : 0L); };
    f32x4 pv[ADAM_N], gv[ADAM_N], mv[ADAM_N], vv[ADAM_N];
#pragma unroll
    for (int n = 0; n < ADAM_N; ++n) {
        const long idx = index_of(n);
        if (ADAM) {
            gv[n] = stream_load4(g + idx);
            mv[n] = stream_load4(m + idx);
            if (TWO) vv[n] = stream_load4(v + idx);
            pv[n] = stream_load4(p + idx);
        } else {
            pv[n] = *(const f32x4*)(p + idx);  // pack only: the masters are already up to date (and just written)
        }
    }
    T* const wd = (T*)tl.wd;
#pragma unroll
    for (int n = 0; n < ADAM_N; ++n) {
        const bool mine = in_tile(n);
        f32x4 w = pv[n];
        if (ADAM) {
            f32x4 s0 = mv[n], s1 = TWO ? vv[n] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = w[j], mj = s0[j], vj = s1[j];
                opt_element<RULE>(pj, CLIP ? clipped_grad(gv[n][j], gs, cv) : gv[n][j], mj, vj, lr_t, b1, b2, eps);
                w[j] = pj, s0[j] = mj, s1[j] = vj;
            }
            if (mine) {
                const long idx = index_of(n);
                stream_store4(m + idx, s0);
                if (TWO) stream_store4(v + idx, s1);
                stream_store4(p + idx, w);
            }
        }
        if (bias) continue;
        if (FMT == 1) w = w * wscale;  // (the operand copies hold wscale * w; the masters are written above)
        const int row = n * ADAM_RPP + ty;
#pragma unroll
        for (int j = 0; j < 4; ++j) lds[row][tx * 4 + j] = w[j];
        if (wd && mine) {
            T* o = wd + ((long)(tl.ci0 + row) * tl.k + (tl.k - 1 - tl.tap)) * (PLANES * tl.cout) + tl.co0 + tx * 4;
            if (PLANES == 3) {
                const u32x2 h = pack_hi4<FMT>(w[0], w[1], w[2], w[3]);
                *(u32x2*)o = h;
                *(u32x2*)(o + tl.cout) = h;
                *(u32x2*)(o + 2 * tl.cout) = pack_lo4<FMT>(w[0], w[1], w[2], w[3]);
            } else if (sizeof(T) == 2) {
                *(u32x2*)o = (u32x2){pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3])};
            } else {
                *(f32x4*)o = w;
            }
        }
    }
    if (bias) return;  // (the same in every thread)
    __syncthreads();
    // transposed store: ADAM_CO_T co rows x 64 ci; thread -> (co = threadIdx / 16 + 16 * n, ci4 = (threadIdx % 16) * 4)
    T* const wf = (T*)tl.wf;
#pragma unroll
    for (int n = 0; n < ADAM_TN; ++n) {
        const int col = (threadIdx.x >> 4) + n * 16;
        const int ci4 = (threadIdx.x & 15) * 4;
        const float a0 = lds[ci4][col], a1 = lds[ci4 + 1][col], a2 = lds[ci4 + 2][col], a3 = lds[ci4 + 3][col];
        if (col >= tl.cols || ci4 >= tl.rows) continue;
        T* o = wf + ((long)(tl.co0 + col) * tl.k + tl.tap) * (PLANES * tl.cin) + tl.ci0 + ci4;
        if (PLANES == 3) {
            const u32x2 h = pack_hi4<FMT>(a0, a1, a2, a3);
            *(u32x2*)o = h;
            *(u32x2*)(o + tl.cin) = h;
            *(u32x2*)(o + 2 * tl.cin) = pack_lo4<FMT>(a0, a1, a2, a3);
        } else if (sizeof(T) == 2) {
            *(u32x2*)o = (u32x2){pack_bf16x2(a0, a1), pack_bf16x2(a2, a3)};
        } else {
            *(f32x4*)o = (f32x4){a0, a1, a2, a3};
        }
    }
}

// one work-group per tile
template <typename T, bool ADAM = true, int PLANES = 1, int FMT = 0, bool CLIP = false, int RULE = SL_OPT_ADAM>
__global__ __launch_bounds__(256) void adam_pack_multi_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v, AdamTable t,
                                                              float lr_t, float b1, float b2, float eps, float wscale = 1.f,
                                                              const float* __restrict__ gscale = nullptr, float cv = 0.f) {
    __shared__ float lds[ADAM_CI_T][ADAM_CO_T + 1];
    const AdamTile tl = adam_tile(t, blockIdx.x);
    if (!ADAM && tl.tap == tl.k) return;  // (the bias block has no operand copy)
    const float gs = (CLIP && gscale) ? *gscale : 1.f;
    adam_pack_tile<T, ADAM, PLANES, FMT, CLIP, RULE>(lds, tl, p, g, m, v, lr_t, b1, b2, eps, wscale, gs, cv);
}

}  // namespace

// the table of a call; *tiles_out: the grid of its launch
static int adam_table_from(const sl_adam_layer* layers, int n_layers, const char* who, AdamTable* t, int* tiles_out) {
    t->n = n_layers;
    long tiles = 0;
    for (int i = 0; i < n_layers; ++i) {
        const sl_adam_layer& L = layers[i];
        SL_CHECK_ARG(L.w_fwd && L.k > 0 && L.cin_pad > 0 && L.cout_pad > 0 && L.cin_pad % 32 == 0 && L.cout_pad % 64 == 0 &&
                         L.offset >= 0 && L.offset % 4 == 0,
                     "%s: layer %d: need w_fwd, cin_pad %% 32 == 0, cout_pad %% 64 == 0, offset %% 4 == 0", who, i);
        t->tile_begin[i] = (int)tiles;
        t->offset[i] = L.offset;
        t->wf[i] = L.w_fwd;
        t->wd[i] = L.w_dgrad;
        t->k[i] = L.k;
        t->cin[i] = L.cin_pad;
        t->cout[i] = L.cout_pad;
        const long nco = (L.cout_pad + ADAM_CO_T - 1) / ADAM_CO_T, nci = (L.cin_pad + ADAM_CI_T - 1) / ADAM_CI_T;
        tiles += nco * nci * L.k + nco;  // (+ the bias tiles)
        SL_CHECK_ARG(tiles < (1L << 30), "%s: layer %d: too many tiles for one launch", who, i);
    }
    t->tile_begin[n_layers] = (int)tiles;
    *tiles_out = (int)tiles;
    return SL_OK;
}

// ---- the host side: coefficients, one dispatch, one launcher per kernel ------------------------------------------------------
namespace {
// what a kernel gets of a rule: built by adam_coeffs or rule_coeffs, which leave their refusal in rc for the launcher to return
struct OptCoeffs {
    int rc, rule;
    float lr, c0, c1, eps;
};
// the buffers of an update and its clipping (grad_scale NULL and clipvalue 0: none, the CLIP = false instantiation)
struct OptArgs {
    float *param;
    const float* grad;
    float *s0, *s1;
    const float* grad_scale;
    float clipvalue;
    void* stream;
};
enum OptOperands { OPERANDS_DTYPE, OPERANDS_BF16X3, OPERANDS_F16X3 };  // which family of fused entry points
}  // namespace

static OptCoeffs no_coeffs(const char* who, const char* why, int rule = 0) {
    sl_set_error(why, who, rule);
    return {SL_ERR_INVALID_ARGUMENT};
}

// Adam (sl_adam_*: they take the step count): the ONE place with Keras 2.0's bias correction, in double
static OptCoeffs adam_coeffs(const char* who, int step, float lr, float beta1, float beta2, float eps) {
    if (step < 1) return no_coeffs(who, "%s: step must be >= 1");
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step));
    return {SL_OK, SL_OPT_ADAM, (float)lr_t, beta1, beta2, eps};
}

// the rules beside Adam (sl_*optimizer_*): lr is the caller's decayed rate
static OptCoeffs rule_coeffs(const char* who, const sl_opt_rule* r) {
    if (r == nullptr) return no_coeffs(who, "%s: null rule");
    switch (r->rule) {
        case SL_OPT_SGD: return {SL_OK, r->rule, r->lr, r->momentum, r->nesterov ? 1.f : 0.f, r->eps};
        case SL_OPT_RMSPROP:
        case SL_OPT_ADADELTA: return {SL_OK, r->rule, r->lr, r->rho, 0.f, r->eps};
        case SL_OPT_ADAGRAD: return {SL_OK, r->rule, r->lr, 0.f, 0.f, r->eps};
        case SL_OPT_ADAMAX: return {SL_OK, r->rule, r->lr, r->beta1, r->beta2, r->eps};
        case SL_OPT_ADAM: return no_coeffs(who, "%s: Adam has its own entry points (sl_adam_*: they take the step count)");
        default: return no_coeffs(who, "%s: unknown rule %d", r->rule);
    }
}

// one switch over the rule ids for every launch of this family: LAUNCH(CLIP, RULE) launches that instantiation
#define SL_OPT_LAUNCH_RULE(RULE, clip, LAUNCH)  \
    case RULE:                                  \
        if (clip) { LAUNCH(true, RULE); } else { LAUNCH(false, RULE); } \
        break;
#define SL_OPT_DISPATCH(rule, clip, LAUNCH)           \
    switch (rule) {                                   \
        SL_OPT_LAUNCH_RULE(SL_OPT_ADAM, clip, LAUNCH)     \
        SL_OPT_LAUNCH_RULE(SL_OPT_SGD, clip, LAUNCH)      \
        SL_OPT_LAUNCH_RULE(SL_OPT_RMSPROP, clip, LAUNCH)  \
        SL_OPT_LAUNCH_RULE(SL_OPT_ADAGRAD, clip, LAUNCH)  \
        SL_OPT_LAUNCH_RULE(SL_OPT_ADADELTA, clip, LAUNCH) \
        SL_OPT_LAUNCH_RULE(SL_OPT_ADAMAX, clip, LAUNCH)   \
        default: break;                               \
    }

// what every update checks of its buffers: a one-slot rule takes no second state pointer (the kernels get NULL for it), Adam
// and the other two-slot rules need both
static int check_opt_args(const char* who, const OptArgs& a, const OptCoeffs& c) {
    if (c.rc != SL_OK) return c.rc;
    SL_CHECK_ARG(a.param && a.grad && a.s0, "%s: null pointer", who);
    SL_CHECK_ARG((a.s1 != nullptr) == opt_two_slots(c.rule),
                 "%s: s1 (Adam: v) is required exactly when the rule keeps two state slots", who);
    SL_CHECK_ARG(a.clipvalue >= 0.f, "%s: clipvalue must be >= 0 (0 = off)", who);
    return SL_OK;
}

// THE flat launch: sl_adam_step, sl_adam_step_clipped, sl_optimizer_step
static int launch_flat(const char* who, const OptArgs& a, size_t n, const OptCoeffs& c) {
    const int rc = check_opt_args(who, a, c);
    if (rc != SL_OK) return rc;
    SL_CHECK_ARG(n % 4 == 0, "%s: n must be a multiple of 4", who);
    const long n4 = (long)(n / 4);
    if (n4 == 0) return SL_OK;
    const dim3 grid((unsigned)((n4 + 255) / 256));
#define SL_OPT_FLAT(CLIP, RULE)                                                                                           \
    hipLaunchKernelGGL((adam_kernel<CLIP, RULE>), grid, dim3(256), 0, (hipStream_t)a.stream, a.param, a.grad, a.s0, a.s1, \
                       n4, c.lr, c.c0, c.c1, c.eps, a.grad_scale, a.clipvalue)
    SL_OPT_DISPATCH(c.rule, a.grad_scale != nullptr || a.clipvalue > 0.f, SL_OPT_FLAT)
#undef SL_OPT_FLAT
    return sl_check_launch(who);
}

// THE fused update + repack launch of the nine *_pack_layers entry points and sl_adam_pack_layer.
// T / PLANES / FMT: the operand format (adam_pack_tile)
template <typename T, int PLANES, int FMT>
static int launch_fused(const char* who, const OptArgs& a, const sl_adam_layer* layers, int n_layers, const OptCoeffs& c,
                        float w_scale) {
    int rc = check_opt_args(who, a, c);
    if (rc != SL_OK) return rc;
    SL_CHECK_ARG(layers && w_scale > 0.f, "%s: null pointer or bad scale", who);
    SL_CHECK_ARG(n_layers >= 1 && n_layers <= SL_ADAM_MAX_LAYERS, "%s: 1..%d layers per call", who, SL_ADAM_MAX_LAYERS);
    AdamTable t;
    int blocks = 0;
    rc = adam_table_from(layers, n_layers, who, &t, &blocks);
    if (rc != SL_OK) return rc;
#define SL_OPT_PACK(CLIP, RULE)                                                                                \
    hipLaunchKernelGGL((adam_pack_multi_kernel<T, true, PLANES, FMT, CLIP, RULE>), dim3(blocks), dim3(256), 0, \
                       (hipStream_t)a.stream, a.param, a.grad, a.s0, a.s1, t, c.lr, c.c0, c.c1, c.eps, w_scale, \
                       a.grad_scale, a.clipvalue)
    SL_OPT_DISPATCH(c.rule, a.grad_scale != nullptr || a.clipvalue > 0.f, SL_OPT_PACK)
#undef SL_OPT_PACK
    return sl_check_launch(who);
}
#undef SL_OPT_DISPATCH
#undef SL_OPT_LAUNCH_RULE

// <T, PLANES, FMT> of an entry point: bf16x3 and f16x3 have entry points of their own, the others say it in `dtype`
static int launch_fused_for(OptOperands operands, int dtype, const char* who, const OptArgs& a, const sl_adam_layer* layers,
                            int n_layers, const OptCoeffs& c, float w_scale = 1.f) {
    if (operands == OPERANDS_DTYPE) {
        SL_CHECK_ARG(dtype == SL_BF16 || dtype == SL_F32, "%s: bad dtype", who);
        if (dtype == SL_BF16) return launch_fused<unsigned short, 1, 0>(who, a, layers, n_layers, c, w_scale);
        return launch_fused<float, 1, 0>(who, a, layers, n_layers, c, w_scale);
    }
    if (operands == OPERANDS_BF16X3) return launch_fused<unsigned short, 3, 0>(who, a, layers, n_layers, c, w_scale);
    return launch_fused<unsigned short, 3, 1>(who, a, layers, n_layers, c, w_scale);
}

// ---- the entry points: their name, their own checks, one call ----------------------------------------------------------------
// A clipped twin called with NULL / 0 launches the plain instantiation -- the original's kernel, hence its bits.
extern "C" int sl_adam_step_clipped(float* param, const float* grad, float* m, float* v, size_t n, int step, float lr,
                                    float beta1, float beta2, float eps, const float* grad_scale, float clipvalue,
                                    void* stream) {
    const char* who = (grad_scale || clipvalue != 0.f) ? "sl_adam_step_clipped" : "sl_adam_step";
    return launch_flat(who, {param, grad, m, v, grad_scale, clipvalue, stream}, n, adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_adam_step(float* param, const float* grad, float* m, float* v, size_t n, int step, float lr,
                            float beta1, float beta2, float eps, void* stream) {
    return sl_adam_step_clipped(param, grad, m, v, n, step, lr, beta1, beta2, eps, nullptr, 0.f, stream);
}

extern "C" int sl_optimizer_step(float* param, const float* grad, float* s0, float* s1, size_t n, const sl_opt_rule* rule,
                                 const float* grad_scale, float clipvalue, void* stream) {
    const char* who = "sl_optimizer_step";
    return launch_flat(who, {param, grad, s0, s1, grad_scale, clipvalue, stream}, n, rule_coeffs(who, rule));
}

extern "C" int sl_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                           int n_layers, int dtype, int step, float lr, float beta1, float beta2, float eps,
                                           const float* grad_scale, float clipvalue, void* stream) {
    const char* who = "sl_adam_pack_layers_clipped";
    return launch_fused_for(OPERANDS_DTYPE, dtype, who, {param, grad, m, v, grad_scale, clipvalue, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                   int n_layers, int dtype, int step, float lr, float beta1, float beta2, float eps,
                                   void* stream) {
    const char* who = "sl_adam_pack_layers";
    return launch_fused_for(OPERANDS_DTYPE, dtype, who, {param, grad, m, v, nullptr, 0.f, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_split3_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v,
                                                  const sl_adam_layer* layers, int n_layers, int step, float lr, float beta1,
                                                  float beta2, float eps, const float* grad_scale, float clipvalue,
                                                  void* stream) {
    const char* who = "sl_split3_adam_pack_layers_clipped";
    return launch_fused_for(OPERANDS_BF16X3, 0, who, {param, grad, m, v, grad_scale, clipvalue, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_split3_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                          int n_layers, int step, float lr, float beta1, float beta2, float eps, void* stream) {
    const char* who = "sl_split3_adam_pack_layers";
    return launch_fused_for(OPERANDS_BF16X3, 0, who, {param, grad, m, v, nullptr, 0.f, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_splitf16_adam_pack_layers_clipped(float* param, const float* grad, float* m, float* v,
                                                    const sl_adam_layer* layers, int n_layers, int step, float lr, float beta1,
                                                    float beta2, float eps, float w_scale, const float* grad_scale,
                                                    float clipvalue, void* stream) {
    const char* who = "sl_splitf16_adam_pack_layers_clipped";
    return launch_fused_for(OPERANDS_F16X3, 0, who, {param, grad, m, v, grad_scale, clipvalue, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps), w_scale);
}

extern "C" int sl_splitf16_adam_pack_layers(float* param, const float* grad, float* m, float* v, const sl_adam_layer* layers,
                                            int n_layers, int step, float lr, float beta1, float beta2, float eps,
                                            float w_scale, void* stream) {
    const char* who = "sl_splitf16_adam_pack_layers";
    return launch_fused_for(OPERANDS_F16X3, 0, who, {param, grad, m, v, nullptr, 0.f, stream}, layers, n_layers,
                            adam_coeffs(who, step, lr, beta1, beta2, eps), w_scale);
}

extern "C" int sl_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1, const sl_adam_layer* layers,
                                        int n_layers, int dtype, const sl_opt_rule* rule, const float* grad_scale,
                                        float clipvalue, void* stream) {
    const char* who = "sl_optimizer_pack_layers";
    return launch_fused_for(OPERANDS_DTYPE, dtype, who, {param, grad, s0, s1, grad_scale, clipvalue, stream}, layers, n_layers,
                            rule_coeffs(who, rule));
}

extern "C" int sl_split3_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1,
                                               const sl_adam_layer* layers, int n_layers, const sl_opt_rule* rule,
                                               const float* grad_scale, float clipvalue, void* stream) {
    const char* who = "sl_split3_optimizer_pack_layers";
    return launch_fused_for(OPERANDS_BF16X3, 0, who, {param, grad, s0, s1, grad_scale, clipvalue, stream}, layers, n_layers,
                            rule_coeffs(who, rule));
}

extern "C" int sl_splitf16_optimizer_pack_layers(float* param, const float* grad, float* s0, float* s1,
                                                 const sl_adam_layer* layers, int n_layers, const sl_opt_rule* rule,
                                                 float w_scale, const float* grad_scale, float clipvalue, void* stream) {
    const char* who = "sl_splitf16_optimizer_pack_layers";
    return launch_fused_for(OPERANDS_F16X3, 0, who, {param, grad, s0, s1, grad_scale, clipvalue, stream}, layers, n_layers,
                            rule_coeffs(who, rule), w_scale);
}

// one layer block (param, grad, m, v point at its first weight): a one-row table through the fused launch -- the same tile
// function over the same tiles.  (any dtype but SL_BF16 means fp32 here)
extern "C" int sl_adam_pack_layer(float* param, const float* grad, float* m, float* v, void* w_fwd, void* w_dgrad, int k,
                                  int cin_pad, int cout_pad, int dtype, int step, float lr, float beta1, float beta2,
                                  float eps, void* stream) {
    const char* who = "sl_adam_pack_layer";
    SL_CHECK_ARG(param && grad && m && v && w_fwd, "%s: null pointer", who);
    SL_CHECK_ARG(k > 0 && cin_pad > 0 && cout_pad > 0 && cin_pad % 32 == 0 && cout_pad % 64 == 0 && step >= 1,
                 "%s: need cin_pad %% 32 == 0, cout_pad %% 64 == 0, step >= 1", who);
    const sl_adam_layer layer = {0, w_fwd, w_dgrad, k, cin_pad, cout_pad};
    return launch_fused_for(OPERANDS_DTYPE, dtype == SL_BF16 ? SL_BF16 : SL_F32, who, {param, grad, m, v, nullptr, 0.f, stream},
                            &layer, 1, adam_coeffs(who, step, lr, beta1, beta2, eps));
}

extern "C" int sl_pack_layers(const float* param, const sl_adam_layer* layers, int n_layers, int dtype, void* stream) {
    SL_CHECK_ARG(param && layers, "sl_pack_layers: null pointer");
    SL_CHECK_ARG(n_layers >= 1 && n_layers <= SL_ADAM_MAX_LAYERS, "sl_pack_layers: 1..%d layers per call",
                 SL_ADAM_MAX_LAYERS);
    SL_CHECK_ARG(dtype == SL_BF16 || dtype == SL_F32, "sl_pack_layers: bad dtype");
    AdamTable t;
    int blocks = 0;
    const int rc = adam_table_from(layers, n_layers, "sl_pack_layers", &t, &blocks);
    if (rc != SL_OK) return rc;
    float* p = const_cast<float*>(param);  // (read only in the pack-only instantiation)
    if (dtype == SL_BF16)
        hipLaunchKernelGGL((adam_pack_multi_kernel<unsigned short, false>), dim3(blocks), dim3(256), 0,
                           (hipStream_t)stream, p, nullptr, nullptr, nullptr, t, 0.f, 0.f, 0.f, 0.f);
    else
        hipLaunchKernelGGL((adam_pack_multi_kernel<float, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p,
                           nullptr, nullptr, nullptr, t, 0.f, 0.f, 0.f, 0.f);
    return sl_check_launch("sl_pack_layers");
}

// ---- squared gradient norm + clip factor (include/speechless_hip.h: "Gradient clipping on the device") ----------------------
namespace {

constexpr int NORM_CHUNK = 16384;  // floats per partial: 16 x 16-byte loads per thread of a 256-thread work-group

struct NormTable {
    int n;
    int chunk_begin[SL_NORM_MAX_RANGES + 1];  // first chunk of range i (chunks count from the range's 4-float-aligned start)
    long offset[SL_NORM_MAX_RANGES], count[SL_NORM_MAX_RANGES];
};

// fixed-order sum of the 256 per-thread doubles of a work-group (tree over LDS); the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double (&red)[256], double acc) {
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// An HBM / L2-bound read: every work-group walks whole chunks (grid-stride; the grid is sized to the CUs, the chunking is
// not, so the partials do not depend on the grid).  Per thread 16 x f32x4 of a chunk, four loads in flight, accumulated in
// double in index order.  The first / last vector of a range may straddle its ends: those take guarded scalar loads (a 16-byte
// load there could also leave the allocation).
__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(const float* __restrict__ g, NormTable t, int n_chunks,
                                                                  double* __restrict__ partial) {
    __shared__ double red[256];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        int r = 0;
        while (r + 1 < t.n && c >= t.chunk_begin[r + 1]) ++r;
        const long lo = t.offset[r], hi = lo + t.count[r];
        const long q0 = (lo >> 2) + (long)(c - t.chunk_begin[r]) * (NORM_CHUNK / 4);  // first f32x4 (absolute) of this chunk
        double acc = 0.0;
#pragma unroll
        for (int u0 = 0; u0 < 16; u0 += 4) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long e = (q0 + (long)(u0 + u) * 256 + threadIdx.x) * 4;
                if (e >= lo && e + 4 <= hi) {
                    v[u] = *(const f32x4*)(g + e);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[u][j] = (e + j >= lo && e + j < hi) ? g[e + j] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = fma((double)v[u][j], (double)v[u][j], acc);
        }
        const double s = block_sum_256(red, acc);
        if (threadIdx.x == 0) partial[c] = s;
        __syncthreads();  // (red is reused by the next chunk)
    }
}

__device__ __forceinline__ void write_clip_scale(double sq, float clipnorm, float* scale, float* norm) {
    const double n = sqrt(sq);
    if (norm) *norm = (float)n;
    if (scale) *scale = (clipnorm > 0.f && n >= (double)clipnorm) ? (float)((double)clipnorm / n) : 1.0f;
}

// one work-group: thread i adds partials i, i + 256, ... in that order, then the tree
__global__ __launch_bounds__(256) void grad_sqnorm_final_kernel(const double* __restrict__ partial, int n, float clipnorm,
                                                                double* __restrict__ sqnorm, float* norm, float* scale) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    const double s = block_sum_256(red, acc);
    if (threadIdx.x == 0) {
        *sqnorm = s;
        write_clip_scale(s, clipnorm, scale, norm);
    }
}

__global__ void clip_scale_kernel(const double* __restrict__ sqnorm, int n_terms, float clipnorm, float* scale, float* norm) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < n_terms; ++i) s += sqnorm[i];
    write_clip_scale(s, clipnorm, scale, norm);
}

int norm_table_from(const sl_norm_range* ranges, int n_ranges, NormTable* t) {
    long chunks = 0;
    t->n = n_ranges;
    for (int i = 0; i < n_ranges; ++i) {
        if (ranges[i].offset < 0 || ranges[i].count < 0) return -1;
        t->chunk_begin[i] = (int)chunks;
        t->offset[i] = ranges[i].offset;
        t->count[i] = ranges[i].count;
        const long span = ranges[i].count ? (ranges[i].offset & 3) + ranges[i].count : 0;  // from the aligned start
        chunks += (span + NORM_CHUNK - 1) / NORM_CHUNK;
        if (chunks > (1L << 30)) return -1;
    }
    t->chunk_begin[n_ranges] = (int)chunks;
    return (int)chunks;
}

}  // namespace

extern "C" size_t sl_grad_sqnorm_workspace_bytes(const sl_norm_range* ranges, int n_ranges) {
    NormTable t;
    if (!ranges || n_ranges < 1 || n_ranges > SL_NORM_MAX_RANGES) return 0;
    const int chunks = norm_table_from(ranges, n_ranges, &t);
    return chunks < 0 ? 0 : (size_t)(chunks > 0 ? chunks : 1) * sizeof(double);
}

extern "C" int sl_grad_sqnorm(const float* grad, const sl_norm_range* ranges, int n_ranges, float clipnorm, double* sqnorm,
                              float* norm, float* scale, void* workspace, size_t workspace_bytes, void* stream) {
    SL_CHECK_ARG(grad && ranges && sqnorm && workspace, "sl_grad_sqnorm: null pointer");
    SL_CHECK_ARG(n_ranges >= 1 && n_ranges <= SL_NORM_MAX_RANGES, "sl_grad_sqnorm: 1..%d ranges per call", SL_NORM_MAX_RANGES);
    SL_CHECK_ARG(((uintptr_t)grad & 15) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sqnorm & 7) == 0,
                 "sl_grad_sqnorm: grad must be 16-byte aligned, workspace and sqnorm 8-byte aligned");
    NormTable t;
    const int chunks = norm_table_from(ranges, n_ranges, &t);
    SL_CHECK_ARG(chunks >= 0, "sl_grad_sqnorm: a range has a negative offset or count (or the table is too long)");
    if (workspace_bytes < (size_t)(chunks > 0 ? chunks : 1) * sizeof(double)) {
        sl_set_error("sl_grad_sqnorm: workspace too small");
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (chunks > 0) {
        const int grid = chunks < sl_cus() * 8 ? chunks : sl_cus() * 8;  // eight 4-wave work-groups per CU hide the HBM latency
        hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(grid), dim3(256), 0, s, grad, t, chunks, (double*)workspace);
        const int rc = sl_check_launch("sl_grad_sqnorm(partial)");
        if (rc != SL_OK) return rc;
    }
    hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, chunks, clipnorm, sqnorm,
                       norm, scale);
    return sl_check_launch("sl_grad_sqnorm(final)");
}

extern "C" int sl_clip_scale(const double* sqnorm, int n_terms, float clipnorm, float* scale, float* norm, void* stream) {
    SL_CHECK_ARG(sqnorm && (scale || norm), "sl_clip_scale: null pointer");
    SL_CHECK_ARG(n_terms >= 1 && n_terms <= 1024, "sl_clip_scale: 1..1024 terms");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sqnorm, n_terms, clipnorm, scale, norm);
    return sl_check_launch("sl_clip_scale");
}
