// asg.hip -- ASG (auto segmentation criterion, Collobert et al. 2016, arXiv:1609.03193) for gfx950: loss, the gradients
// w.r.t. the output layer's logits, the transition scores and the start scores, and the Viterbi decode over the full graph.
//
// No reference counterpart: the reference raises NotImplementedError where its ASG loss would be (speechless/net.py:397-399).
// Semantics: include/speechless_hip.h, sl_asg_loss_grad / sl_asg_viterbi ("ASG criterion").
//
// sl_asg_loss_grad is four launches on one stream, every sum in a fixed order (no float atomics: bitwise reproducible):
//   asg_lattice_kernel<NS>  grid (B, 4), ONE WAVE per utterance and role, T' sequential frames each:
//     role 0 / 1  numerator alpha / beta over the label's L states in the LOG domain, in doubles (NS = 1 / 2 / 4 / 8
//                 consecutive states per lane in registers; the neighbour state of the lane below / above by one shuffle).
//                 A probability-domain lattice would lose whole utterances here: with a collapsed distribution the
//                 states of one frame differ by more than the range of a double.
//     role 2 / 3  denominator alpha / beta over the K letters in the PROBABILITY domain, in doubles, lane j owning letter
//                 j: exp(g) sits in LDS ([from][to] for alpha, [to][from] for beta, so that a lane's reads are
//                 conflict-free), a frame is K multiply-adds per lane and one rescale by the frame's sum.  One frame
//                 changes a value by a factor in [eps e^-|g|, e^|g|], so a rescale per frame keeps everything inside the range
//                 of a double whatever the distribution; log Z is the sum of the logs of the alpha scales (one log per frame
//                 instead of K^2 exp).
//   asg_grad_kernel         one wave per frame: the state posteriors of both lattices, G = gamma_den - gamma_num, the
//                           softmax chain, the row of dlogits (zeros for t >= T_b), the loss, the utterance's dinit row.
//   asg_trans_kernel        one work-group per utterance: the pair posteriors summed over the frames, [K][K] per utterance.
//   asg_reduce_kernel       dtrans / dinit = grad_scale * the per-utterance partials summed over b = 0 .. B-1 in that order.
// Emissions are log(p + eps) from probs, in doubles (the per-frame constant by which logq differs cancels in Z - N).
//
// sl_asg_viterbi: one wave per utterance, lane j owning letter j, fp32; per frame K compare-and-adds per lane against the
// previous frame's scores in LDS (a broadcast read) and the transition column in LDS; one byte of backpointer per letter
// and frame, in LDS when T' * K bytes fit, else in the workspace.
#include <math.h>

#include "lattice.h"

namespace {

constexpr int CH = 8;    // frames of emissions per staging chunk
constexpr int FR = 8;    // frames per LDS chunk of asg_trans_kernel
constexpr int NP = 16;   // letter pairs per thread of asg_trans_kernel: 64 * 64 / 256
constexpr int VIT_LDS_MAX = 128 * 1024;

struct AsgLayout {
    size_t la, lb, em, da, db, cfac, wnorm, scal, ptrans, pinit, total;
};

AsgLayout asg_layout(int batch, int t_out, int k, int l_max) {
    const size_t lm = l_max < 1 ? 1 : l_max;
    const size_t bt = (size_t)batch * t_out;
    AsgLayout w;
    size_t off = 0;
    auto take = [&](size_t doubles) {
        const size_t o = off;
        off += doubles * sizeof(double);
        return o;
    };
    w.la = take(bt * lm);
    w.lb = take(bt * lm);
    w.em = take(bt * k);
    w.da = take(bt * k);
    w.db = take(bt * k);
    w.cfac = take(bt);
    w.wnorm = take(bt);
    w.scal = take((size_t)batch * 2);  // N, log Z
    w.ptrans = take((size_t)batch * k * k);
    w.pinit = take((size_t)batch * k);
    w.total = off;
    return w;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double lse2(double x, double y) {
    const double m = fmax(x, y);
    if (m == -INFINITY) return m;
    return m + log1p(exp(fmin(x, y) - m));
}

// ---------------------------------------------------------------------------------------------- numerator lattices
// smem: [CH][64] doubles of emissions
template <int NS, bool BETA>
__device__ __forceinline__ void numerator_lattice(double* smem, const float* __restrict__ probs, const float* __restrict__ trans,
                                                  const float* __restrict__ init, const int32_t* __restrict__ lab, double* out,
                                                  double* em_ws, double* scal, int L, int T, int k, int lm, double eps) {
    const int lane = threadIdx.x;
    double* em = smem;
    int col[NS];
    double gs[NS], ga[NS], a[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int s = lane * NS + j;
        col[j] = 0;
        gs[j] = 0.0;
        ga[j] = -INFINITY;
        a[j] = -INFINITY;
        if (s < L) {
            const int c = clamp_label(lab[s], k);
            col[j] = c;
            gs[j] = (double)trans[c * k + c];
            if (!BETA && s > 0) ga[j] = (double)trans[clamp_label(lab[s - 1], k) * k + c];  // into s from s - 1
            if (BETA && s + 1 < L) ga[j] = (double)trans[c * k + clamp_label(lab[s + 1], k)];  // out of s into s + 1
            if (BETA && s == L - 1) a[j] = 0.0;
        }
    }
    const bool col_on = lane < k;
    const int nchunks = (T + CH - 1) / CH;
    float pre[CH];
    {
        const int t0 = (BETA ? nchunks - 1 : 0) * CH;
#pragma unroll
        for (int f = 0; f < CH; ++f) {
            const int t = t0 + f < T ? t0 + f : T - 1;
            pre[f] = col_on ? probs[(long)t * k + lane] : 1.f;
        }
    }
    if (BETA) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int s = lane * NS + j;
            if (s < L) out[(long)(T - 1) * lm + s] = a[j];
        }
    }
    for (int ci = 0; ci < nchunks; ++ci) {
        const int c = BETA ? nchunks - 1 - ci : ci;
        const int t0 = c * CH;
        __syncthreads();
#pragma unroll
        for (int f = 0; f < CH; ++f) {
            const double e = log((double)pre[f] + eps);
            em[f * 64 + lane] = e;
            if (!BETA && col_on && t0 + f < T) em_ws[(long)(t0 + f) * k + lane] = e;
        }
        __syncthreads();
        if (ci + 1 < nchunks) {
            const int n0 = (BETA ? c - 1 : c + 1) * CH;
#pragma unroll
            for (int f = 0; f < CH; ++f) {
                const int t = n0 + f < T ? n0 + f : T - 1;
                pre[f] = col_on ? probs[(long)t * k + lane] : 1.f;
            }
        }
        const int nf = T - t0 < CH ? T - t0 : CH;
        if (!BETA) {
            for (int f = 0; f < nf; ++f) {
                const int t = t0 + f;
                const double* e = em + f * 64;
                if (t == 0) {
                    if (lane == 0) a[0] = (double)init[col[0]] + e[col[0]];
                } else {
                    double lo = __shfl_up(a[NS - 1], 1);
                    if (lane == 0) lo = -INFINITY;
#pragma unroll
                    for (int j = NS - 1; j >= 0; --j) {  // descending: a[j - 1] still holds frame t - 1
                        const double prev = j >= 1 ? a[j - 1] : lo;
                        a[j] = e[col[j]] + lse2(a[j] + gs[j], prev + ga[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int s = lane * NS + j;
                    if (s < L) out[(long)t * lm + s] = a[j];
                }
            }
        } else {
            for (int f = nf - 1; f >= 0; --f) {
                const int u = t0 + f;  // beta of frame u - 1 from beta and emissions of frame u
                if (u == 0) break;
                const double* e = em + f * 64;
                double uu[NS];
#pragma unroll
                for (int j = 0; j < NS; ++j) uu[j] = a[j] + e[col[j]];
                double hi = __shfl_down(uu[0], 1);
                if (lane == 63) hi = -INFINITY;
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const double nxt = j + 1 < NS ? uu[j + 1] : hi;
                    a[j] = lse2(uu[j] + gs[j], nxt + ga[j]);
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int s = lane * NS + j;
                    if (s < L) out[(long)(u - 1) * lm + s] = a[j];
                }
            }
        }
    }
    if (!BETA) {
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (lane * NS + j == L - 1) scal[0] = a[j];
    }
}

// ---------------------------------------------------------------------------------------------- denominator lattices
// smem: [k][k] doubles of exp(g) ([from][to] for alpha, [to][from] for beta), then 64 doubles of the previous frame
template <bool BETA>
__device__ __forceinline__ void denominator_lattice(double* smem, const float* __restrict__ probs, const float* __restrict__ trans,
                                                    const float* __restrict__ init, double* out, double* cfac, double* scal,
                                                    int T, int k, double eps) {
    const int lane = threadIdx.x;
    double* G = smem;
    double* vec = smem + k * k;
    for (int idx = lane; idx < k * k; idx += 64) {
        const int i = idx / k, j = idx - i * k;
        G[BETA ? j * k + i : idx] = exp((double)trans[idx]);
    }
    const bool on = lane < k;
    const int lj = on ? lane : 0;
    const int nchunks = (T + CH - 1) / CH;
    float pre[CH];
    {
        const int t0 = (BETA ? nchunks - 1 : 0) * CH;
#pragma unroll
        for (int f = 0; f < CH; ++f) {
            const int t = t0 + f < T ? t0 + f : T - 1;
            pre[f] = on ? probs[(long)t * k + lane] : 0.f;
        }
    }
    double v = 0.0, logz = 0.0;
    if (BETA) {
        v = on ? 1.0 : 0.0;
        if (on) out[(long)(T - 1) * k + lane] = v;
    }
    for (int ci = 0; ci < nchunks; ++ci) {
        const int c = BETA ? nchunks - 1 - ci : ci;
        const int t0 = c * CH;
        float cur[CH];
#pragma unroll
        for (int f = 0; f < CH; ++f) cur[f] = pre[f];
        if (ci + 1 < nchunks) {
            const int n0 = (BETA ? c - 1 : c + 1) * CH;
#pragma unroll
            for (int f = 0; f < CH; ++f) {
                const int t = n0 + f < T ? n0 + f : T - 1;
                pre[f] = on ? probs[(long)t * k + lane] : 0.f;
            }
        }
        const int nf = T - t0 < CH ? T - t0 : CH;
#pragma unroll
        for (int ff = 0; ff < CH; ++ff) {
            const int f = BETA ? CH - 1 - ff : ff;
            if (f >= nf) continue;  // (wave-uniform)
            const int t = t0 + f;
            const double P = on ? (double)cur[f] + eps : 0.0;
            if (!BETA) {
                double raw;
                if (t == 0) {
                    raw = on ? exp((double)init[lane]) * P : 0.0;
                } else {
                    __syncthreads();
                    vec[lane] = v;
                    __syncthreads();
                    double acc = 0.0;
                    for (int i = 0; i < k; ++i) acc += vec[i] * G[i * k + lj];
                    raw = acc * P;  // (P = 0 on the lanes beyond k)
                }
                const double cs = wave_sum_d(raw);
                v = raw / cs;
                logz += log(cs);
                if (on) out[(long)t * k + lane] = v;
                if (lane == 0) cfac[t] = cs;
            } else {
                if (t == 0) continue;  // beta of frame t - 1 from frame t
                __syncthreads();
                vec[lane] = P * v;
                __syncthreads();
                double acc = 0.0;
                for (int j = 0; j < k; ++j) acc += G[j * k + lj] * vec[j];
                acc = on ? acc : 0.0;
                const double cs = wave_sum_d(acc);
                v = acc / cs;
                if (on) out[(long)(t - 1) * k + lane] = v;
            }
        }
    }
    if (!BETA && lane == 0) scal[1] = logz;
}

template <int NS>
__global__ __launch_bounds__(64) void asg_lattice_kernel(const float* __restrict__ probs, const float* __restrict__ trans,
                                                          const float* __restrict__ init, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ label_len,
                                                          const int32_t* __restrict__ input_len, char* __restrict__ ws,
                                                          AsgLayout w, int t_out, int k, int l_max, float eps_f) {
    extern __shared__ double smem_d[];
    const int b = blockIdx.x;
    const int role = blockIdx.y;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    if (L == 0 || T == 0 || L > T) return;  // infeasible: asg_grad_kernel / asg_trans_kernel decide the same way
    const int lm = l_max < 1 ? 1 : l_max;
    const double eps = (double)eps_f;
    const float* p = probs + (long)b * t_out * k;
    const int32_t* lab = labels + (long)b * l_max;
    double* scal = (double*)(ws + w.scal) + (long)b * 2;
    double* em_ws = (double*)(ws + w.em) + (long)b * t_out * k;
    if (role == 0)
        numerator_lattice<NS, false>(smem_d, p, trans, init, lab, (double*)(ws + w.la) + (long)b * t_out * lm, em_ws, scal, L, T, k,
                                     lm, eps);
    else if (role == 1)
        numerator_lattice<NS, true>(smem_d, p, trans, init, lab, (double*)(ws + w.lb) + (long)b * t_out * lm, em_ws, scal, L, T, k,
                                    lm, eps);
    else if (role == 2)
        denominator_lattice<false>(smem_d, p, trans, init, (double*)(ws + w.da) + (long)b * t_out * k,
                                   (double*)(ws + w.cfac) + (long)b * t_out, scal, T, k, eps);
    else
        denominator_lattice<true>(smem_d, p, trans, init, (double*)(ws + w.db) + (long)b * t_out * k, nullptr, scal, T, k, eps);
}

// ---------------------------------------------------------------------------------------------- per-frame gradient
// 4 waves per work-group, one frame each.  smem: [lm] ints (labels), then 4 x [lm] doubles (a wave's state posteriors)
__global__ __launch_bounds__(256) void asg_grad_kernel(const float* __restrict__ probs, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ label_len,
                                                        const int32_t* __restrict__ input_len, float* __restrict__ loss,
                                                        void* __restrict__ dlogits, char* __restrict__ ws, AsgLayout w, int t_out,
                                                        int k, int l_max, int g_row0, int g_rs, long g_bs, int out_f32,
                                                        float eps_f, float grad_scale) {
    extern __shared__ double smem_d[];
    const int lm = l_max < 1 ? 1 : l_max;
    double* gam_all = smem_d;
    int* s_lab = (int*)(smem_d + 4 * lm);
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    const bool feasible = !(L == 0 || T == 0 || L > T);
    for (int s = threadIdx.x; s < L; s += 256) s_lab[s] = clamp_label(labels[(long)b * l_max + s], k);
    __syncthreads();
    if (t >= t_out) return;
    double* pinit = (double*)(ws + w.pinit) + (long)b * k;
    float dz = 0.f;
    if (feasible && t < T) {
        const double* scal = (const double*)(ws + w.scal) + (long)b * 2;
        const double N = scal[0], logz = scal[1];
        const long row = (long)b * t_out + t;
        const bool on = lane < k;
        // denominator: gamma_t(j) = A_t(j) B_t(j) / sum_j A_t(j) B_t(j) (the posteriors of a frame sum to 1: no scales needed)
        const double prod = on ? ((const double*)(ws + w.da))[row * k + lane] * ((const double*)(ws + w.db))[row * k + lane] : 0.0;
        const double S = wave_sum_d(prod);
        if (lane == 0) ((double*)(ws + w.wnorm))[row] = 1.0 / (((const double*)(ws + w.cfac))[row] * S);
        // numerator: states inside the band that can be occupied at frame t
        const int s_lo = (L - 1) - (T - 1 - t) > 0 ? (L - 1) - (T - 1 - t) : 0;
        const int s_hi = t < L - 1 ? t : L - 1;
        double* gam = gam_all + wave * lm;
        const double* la = (const double*)(ws + w.la) + row * lm;
        const double* lb = (const double*)(ws + w.lb) + row * lm;
        for (int s = s_lo + lane; s <= s_hi; s += 64) gam[s] = exp(la[s] + lb[s] - N);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        double gnum = 0.0;
        if (on)
            for (int s = s_lo; s <= s_hi; ++s)
                if (s_lab[s] == lane) gnum += gam[s];
        const double G = prod / S - gnum;
        const double p = on ? (double)probs[row * k + lane] : 0.0;
        const double x = on ? G * (p / (p + (double)eps_f)) : 0.0;
        const double inner = wave_sum_d(x);
        dz = (float)((double)grad_scale * (x - p * inner));
        if (t == 0) {
            if (on) pinit[lane] = G;
            if (lane == 0) loss[b] = (float)(logz - N);
        }
    } else if (!feasible && t == 0) {
        if (lane < k) pinit[lane] = 0.0;
        if (lane == 0) loss[b] = INFINITY;
    }
    if (dlogits != nullptr && lane < k) {
        const long gi = (long)b * g_bs + (long)(g_row0 + t) * g_rs + lane;
        if (out_f32)
            ((float*)dlogits)[gi] = dz;
        else
            ((unsigned short*)dlogits)[gi] = f32_to_bf16_bits(dz);
    }
}

// ---------------------------------------------------------------------------------------------- pair posteriors
// smem doubles: [FR][64] X (A_{t-1}), [FR][64] Y (P_t B_t / (c_t S_t)), [lm] stay sums, [lm] advance sums; then [lm] ints
__global__ __launch_bounds__(256) void asg_trans_kernel(const float* __restrict__ probs, const float* __restrict__ trans,
                                                         const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ label_len,
                                                         const int32_t* __restrict__ input_len, char* __restrict__ ws, AsgLayout w,
                                                         int t_out, int k, int l_max, float eps_f) {
    extern __shared__ double smem_d[];
    const int lm = l_max < 1 ? 1 : l_max;
    double* X = smem_d;
    double* Y = X + FR * 64;
    double* stay = Y + FR * 64;
    double* adv = stay + lm;
    int* s_lab = (int*)(adv + lm);
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int kk = k * k;
    double* part = (double*)(ws + w.ptrans) + (long)b * kk;
    int L, T;
    clamp_lengths(label_len, input_len, b, l_max, t_out, L, T);
    if (L == 0 || T == 0 || L > T) {
        for (int p = tid; p < kk; p += 256) part[p] = 0.0;
        return;
    }
    for (int s = tid; s < L; s += 256) s_lab[s] = clamp_label(labels[(long)b * l_max + s], k);
    __syncthreads();
    const double N = ((const double*)(ws + w.scal))[(long)b * 2];
    const long row0 = (long)b * t_out;
    const double* la = (const double*)(ws + w.la) + row0 * lm;
    const double* lb = (const double*)(ws + w.lb) + row0 * lm;
    const double* em = (const double*)(ws + w.em) + row0 * k;
    // numerator: the stay (s -> s) and advance (s - 1 -> s) posteriors of state s summed over the frames of its band
    for (int s = tid; s < L; s += 256) {
        const int c = s_lab[s];
        const double gs = (double)trans[c * k + c];
        const double ga = s > 0 ? (double)trans[s_lab[s - 1] * k + c] : 0.0;
        double ss = 0.0, as = 0.0;
        const int t_hi = T - L + s;  // the last frame at which s can still reach the end
        for (int t = s > 1 ? s : 1; t <= t_hi; ++t) {
            const double base = em[(long)t * k + c] + lb[(long)t * lm + s] - N;
            ss += exp(la[(long)(t - 1) * lm + s] + gs + base);
            if (s > 0) as += exp(la[(long)(t - 1) * lm + s - 1] + ga + base);
        }
        stay[s] = ss;
        adv[s] = as;
    }
    // denominator: sum over t of the outer products A_{t-1} (x) Y_t, times exp(g) at the end
    const double* da = (const double*)(ws + w.da) + row0 * k;
    const double* db = (const double*)(ws + w.db) + row0 * k;
    const double* wn = (const double*)(ws + w.wnorm) + row0;
    int pi[NP], pj[NP];
    double acc[NP];
#pragma unroll
    for (int m = 0; m < NP; ++m) {
        const int p = tid + 256 * m;
        const int i = p < kk ? p / k : 0;
        pi[m] = i;
        pj[m] = p < kk ? p - i * k : 0;
        acc[m] = 0.0;
    }
    for (int t0 = 1; t0 < T; t0 += FR) {
        __syncthreads();
        for (int idx = tid; idx < FR * 64; idx += 256) {
            const int f = idx >> 6, c = idx & 63;
            const int t = t0 + f;
            double x = 0.0, y = 0.0;
            if (t < T && c < k) {
                x = da[(long)(t - 1) * k + c];
                y = ((double)probs[(row0 + t) * k + c] + (double)eps_f) * db[(long)t * k + c] * wn[t];
            }
            X[idx] = x;
            Y[idx] = y;
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < FR; ++f)
#pragma unroll
            for (int m = 0; m < NP; ++m) acc[m] += X[f * 64 + pi[m]] * Y[f * 64 + pj[m]];
    }
#pragma unroll
    for (int m = 0; m < NP; ++m) acc[m] *= exp((double)trans[tid + 256 * m < kk ? tid + 256 * m : 0]);
    __syncthreads();  // (stay / adv of every state are written)
    for (int s = 0; s < L; ++s) {
        const int c = s_lab[s];
        const int cp = s > 0 ? s_lab[s - 1] : -1;
        const double ss = stay[s], as = adv[s];
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            if (pj[m] == c) {
                if (pi[m] == c) acc[m] -= ss;
                if (pi[m] == cp) acc[m] -= as;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < NP; ++m) {
        const int p = tid + 256 * m;
        if (p < kk) part[p] = acc[m];
    }
}

__global__ __launch_bounds__(256) void asg_reduce_kernel(const char* __restrict__ ws, AsgLayout w, float* __restrict__ dtrans,
                                                          float* __restrict__ dinit, int batch, int k, float grad_scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int kk = k * k;
    if (idx >= kk + k) return;
    const bool is_init = idx >= kk;
    const double* src = is_init ? (const double*)(ws + w.pinit) + (idx - kk) : (const double*)(ws + w.ptrans) + idx;
    const long stride = is_init ? k : kk;
    double sum = 0.0;
    for (int b = 0; b < batch; ++b) sum += src[(long)b * stride];
    const float out = (float)((double)grad_scale * sum);
    if (is_init)
        dinit[idx - kk] = out;
    else
        dtrans[idx] = out;
}

// ---------------------------------------------------------------------------------------------- Viterbi
// smem: [k][k] floats (g), 64 floats (previous frame), then the backpointer rows (BP_LDS)
template <bool BP_LDS>
__global__ __launch_bounds__(64) void asg_viterbi_kernel(const float* __restrict__ emis, const float* __restrict__ trans,
                                                          const float* __restrict__ init,
                                                          const int32_t* __restrict__ input_len, int32_t* __restrict__ path,
                                                          float* __restrict__ score, uint8_t* __restrict__ bp_hbm, int t_out,
                                                          int k) {
    extern __shared__ float smem_f[];
    float* tr = smem_f;
    float* vs = tr + k * k;
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    uint8_t* bp = BP_LDS ? (uint8_t*)(vs + 64) : bp_hbm + (long)b * t_out * k;
    int T = input_len[b];
    T = T < 0 ? 0 : (T > t_out ? t_out : T);
    int32_t* prow = path + (long)b * t_out;
    for (int t = T + lane; t < t_out; t += 64) prow[t] = -1;
    if (T == 0) {
        if (lane == 0) score[b] = -INFINITY;
        return;
    }
    for (int idx = lane; idx < k * k; idx += 64) tr[idx] = trans[idx];
    const bool on = lane < k;
    const int lj = on ? lane : 0;
    const float* e = emis + (long)b * t_out * k;
    float v = on ? init[lane] + e[lane] : -INFINITY;
    float e_next = (on && T > 1) ? e[k + lane] : 0.f;
    for (int t = 1; t < T; ++t) {
        __syncthreads();
        vs[lane] = v;
        __syncthreads();
        const float et = e_next;
        if (on && t + 1 < T) e_next = e[(long)(t + 1) * k + lane];
        float best = vs[0] + tr[lj];
        int arg = 0;
        for (int i = 1; i < k; ++i) {
            const float c = vs[i] + tr[i * k + lj];
            if (c > best) {
                best = c;
                arg = i;
            }
        }
        v = on ? best + et : -INFINITY;
        if (on) bp[(long)t * k + lane] = (uint8_t)arg;
    }
    __syncthreads();
    vs[lane] = v;
    if (!BP_LDS) __threadfence();
    __syncthreads();
    int s = 0;
    float best = vs[0];
    for (int i = 1; i < k; ++i)
        if (vs[i] > best) {
            best = vs[i];
            s = i;
        }
    if (lane == 0) score[b] = best;
    for (int t = T - 1; t >= 0; --t) {  // (every lane follows the same state: broadcast reads)
        if (lane == 0) prow[t] = s;
        if (t > 0) s = bp[(long)t * k + s];
    }
}

size_t viterbi_lds_bytes(int t_out, int k, bool bp_lds) {
    return (size_t)(k * k + 64) * sizeof(float) + (bp_lds ? (size_t)t_out * k : 0);
}

template <int NS>
void launch_lattice(const float* probs, const float* trans, const float* init, const int32_t* labels, const int32_t* label_len,
                    const int32_t* input_len, char* ws, const AsgLayout& w, int batch, int t_out, int k, int l_max, float eps,
                    hipStream_t s) {
    const size_t den = (size_t)(k * k + 64) * sizeof(double), num = (size_t)CH * 64 * sizeof(double);
    hipLaunchKernelGGL((asg_lattice_kernel<NS>), dim3(batch, 4), dim3(64), den > num ? den : num, s, probs, trans, init, labels,
                       label_len, input_len, ws, w, t_out, k, l_max, eps);
}

}  // namespace

size_t asg_workspace_bytes(int batch, int t_out, int k, int l_max) { return asg_layout(batch, t_out, k, l_max).total; }

int asg_loss_grad(const float* probs, const float* trans, const float* init, const int32_t* labels, const int32_t* label_len,
                  const int32_t* input_len, float* loss, void* dlogits, float* dtrans, float* dinit, int batch, int t_out, int k,
                  int l_max, int g_row0, int g_row_stride, long g_batch_stride, int dtype, float eps, float grad_scale,
                  void* workspace, hipStream_t s) {
    const AsgLayout w = asg_layout(batch, t_out, k, l_max);
    char* ws = (char*)workspace;
    const int lm = l_max < 1 ? 1 : l_max;
    if (lm <= 64)
        launch_lattice<1>(probs, trans, init, labels, label_len, input_len, ws, w, batch, t_out, k, l_max, eps, s);
    else if (lm <= 128)
        launch_lattice<2>(probs, trans, init, labels, label_len, input_len, ws, w, batch, t_out, k, l_max, eps, s);
    else if (lm <= 256)
        launch_lattice<4>(probs, trans, init, labels, label_len, input_len, ws, w, batch, t_out, k, l_max, eps, s);
    else
        launch_lattice<8>(probs, trans, init, labels, label_len, input_len, ws, w, batch, t_out, k, l_max, eps, s);
    int rc = sl_check_launch("sl_asg_loss_grad (lattices)");
    if (rc != SL_OK) return rc;
    const size_t lds_grad = (size_t)4 * lm * sizeof(double) + (size_t)lm * sizeof(int);
    hipLaunchKernelGGL(asg_grad_kernel, dim3((t_out + 3) / 4, batch), dim3(256), lds_grad, s, probs, labels, label_len, input_len,
                       loss, dlogits, ws, w, t_out, k, l_max, g_row0, g_row_stride, g_batch_stride, dtype == SL_F32 ? 1 : 0, eps,
                       grad_scale);
    rc = sl_check_launch("sl_asg_loss_grad (gradient)");
    if (rc != SL_OK || dtrans == nullptr) return rc;
    const size_t lds_tr = (size_t)(2 * FR * 64 + 2 * lm) * sizeof(double) + (size_t)lm * sizeof(int);
    hipLaunchKernelGGL(asg_trans_kernel, dim3(batch), dim3(256), lds_tr, s, probs, trans, labels, label_len, input_len, ws, w,
                       t_out, k, l_max, eps);
    hipLaunchKernelGGL(asg_reduce_kernel, dim3((k * k + k + 255) / 256), dim3(256), 0, s, (const char*)ws, w, dtrans, dinit, batch,
                       k, grad_scale);
    return sl_check_launch("sl_asg_loss_grad (transitions)");
}

size_t asg_viterbi_workspace_bytes(int batch, int t_out, int k) {
    return viterbi_lds_bytes(t_out, k, true) <= (size_t)VIT_LDS_MAX ? 0 : (size_t)batch * t_out * k;
}

int asg_viterbi(const float* emis, const float* trans, const float* init, const int32_t* input_len, int32_t* path, float* score,
                int batch, int t_out, int k, void* workspace, hipStream_t s) {
    const bool bp_lds = asg_viterbi_workspace_bytes(batch, t_out, k) == 0;
    if (bp_lds) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute((const void*)asg_viterbi_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      VIT_LDS_MAX);
            attr_set = true;
        }
        hipLaunchKernelGGL((asg_viterbi_kernel<true>), dim3(batch), dim3(64), viterbi_lds_bytes(t_out, k, true), s, emis, trans,
                           init, input_len, path, score, (uint8_t*)nullptr, t_out, k);
    } else {
        hipLaunchKernelGGL((asg_viterbi_kernel<false>), dim3(batch), dim3(64), viterbi_lds_bytes(t_out, k, false), s, emis, trans,
                           init, input_len, path, score, (uint8_t*)workspace, t_out, k);
    }
    return sl_check_launch("sl_asg_viterbi");
}
