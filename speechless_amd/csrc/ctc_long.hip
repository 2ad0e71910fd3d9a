// ctc_long.hip -- the CTC loss and gradient of ctc.hip for what its wave lattice does not take: labels of 256 .. 2047 letters
// (513 .. 4095 lattice states), and 64 classes at any label length (l_max >= 1: a single wave of 64 threads up to 63 letters).
//
// Same semantics, arguments and outputs as the kernels of ctc.hip (sl_ctc_loss_grad dispatches on l_max and k, host code only);
// the wave lattice there holds a row of up to 511 states in one wave and has a lane per class for 63 classes and the blank's sum.  Generalised from that
// file's repair pass (repair_lattices + ctc_grad_frames<8, 4>: a log-domain lattice in doubles, several states per thread, and
// the gradient pass that reads such rows), as kernels of their own:
//   ctc_long_lattice_kernel<NS> : grid (B, 3) like ctc_lattice_kernel.  Work-group (b,0) runs alpha forwards, (b,1) beta
//                         backwards at the same time, (b,2) builds the per-class position lists.  Up to 1024 threads, each
//                         owning NS CONSECUTIVE states (NS = 2: l_max up to 1023, NS = 4: 1024 .. 2047) in registers; only the
//                         states at a thread's edge cross threads (alpha: one value up, beta: two values down), through
//                         double-buffered LDS rows with one LDS-only barrier per frame.  Emissions are fetched a chunk of 8
//                         frames ahead.  Rows in log2 units, doubles, -inf padding up to the row stride lattice_sp(l_max).
//   ctc_long_grad_kernel : one wave per frame as ctc_grad_kernel, but looping over the row in chunks of 64 columns instead of
//                         keeping sp / 64 columns per lane in registers (64 at sp = 4096).  Same formulas, same fixed summation
//                         order, same destination.  No tickets, no repair pass: the lattice is the accurate one already.
#include "common.h"
#include "ctc_shared.h"
#include "lse_double.h"

namespace {

constexpr double NEG_INF = NEG_INF_D;  // (LOG2E_D, LN2_D and the lse2_long / lse3_long step: lse_double.h)
constexpr int LONG_THREADS_MAX = 1024;
constexpr int LONG_DUMP_DOUBLES = 64 * 4;  // per (utterance, direction): the NS <= 4 states of the <= 63 dead lanes of the last wave

// One direction (DIR 0: alpha, forwards; 1: beta, backwards) of utterance b by the whole work-group.  Thread tid owns the states
// NS * tid .. NS * tid + NS - 1: even offsets are blanks, odd offsets the label positions NS / 2 * tid + i.
//   alpha(s) reads s, s - 1 and (skip) s - 2 of the previous row: beyond its own states a thread needs only its lower
//            neighbour's TOP state (its own lowest state is a blank: no skip into it);
//   beta(s)  reads s, s + 1 and (skip) s + 2: its upper neighbour's two LOWEST states.
// edge: [2][(threads + 2) * EW] doubles, slot tid + 1 (slots 0 and threads + 1: -inf for good).
template <int NS, int DIR>
__device__ __forceinline__ void long_lattice_run(const float* __restrict__ lq_b, const int32_t* __restrict__ lab, int L, int S,
                                                 int T, int k, int blank, int sp, double* __restrict__ rows,
                                                 double* __restrict__ dump, double* edge, double* fin) {
    constexpr int NL = NS / 2;            // label states per thread
    constexpr int EW = DIR == 0 ? 1 : 2;  // values a thread hands to its neighbour
    constexpr int NB = DIR == 0 ? -1 : 1;
    constexpr int OFF = DIR == 0 ? 2 : 0;  // where the thread's own states start in x[] below
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const int s0 = NS * tid;
    int col[NL + 1];
    bool skip[NL], live[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) live[i] = s0 + i < S;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int pos = NL * tid + i;
        const int me = pos < L ? lab[pos] : blank;
        col[i] = me;
        if (DIR == 0)
            skip[i] = pos < L && pos >= 1 && lab[pos - 1] != me;
        else
            skip[i] = pos + 1 < L && lab[pos + 1] != me;
    }
    // the blank's column, per lane like the others: a wave-uniform address would become a scalar load, which the per-frame
    // s_waitcnt lgkmcnt(0) in front of the barrier would wait for
    col[NL] = blank;
    asm volatile("" : "+v"(col[NL]));

    const int bstride = (nt + 2) * EW;  // (the two edge rows are addressed by offset: a selected pointer becomes a flat access)
    if (tid < 2) {
#pragma unroll
        for (int e = 0; e < EW; ++e) {
            edge[tid * (nt + 1) * EW + e] = NEG_INF;
            edge[bstride + tid * (nt + 1) * EW + e] = NEG_INF;
        }
        fin[tid] = NEG_INF;
    }
    __syncthreads();

    const int tstart = DIR == 0 ? 0 : T - 1;
    const int tstep = DIR == 0 ? 1 : -1;
    // every store is unconditional (an exec-masked store between a prefetch load and its use makes the compiler drain
    // vmcnt(0)): the lanes of the last wave beyond the row's end write to a dump slice with stride 0
    const bool in_row = s0 < sp;
    double* outp = in_row ? rows + (long)tstart * sp + s0 : dump + (s0 - sp);
    const long row_inc = in_row ? (long)tstep * sp : 0;

    // Emissions: raw log q values, one chunk of 8 frames AHEAD, consumed (and scaled to log2 units) a chunk later.  Loads at
    // the top of the iteration, the chunk pinned at its bottom, where the compiler can count the younger stores exactly
    // (ctc_lattice_kernel's lessons from the ISA).  Steps past the end re-read the last frame.
    auto load_e = [&](int step, float* e) {
        const int st = step < T ? step : T - 1;
        const float* row = lq_b + (long)(tstart + tstep * st) * k;
#pragma unroll
        for (int i = 0; i <= NL; ++i) e[i] = row[col[i]];
    };
    float ec[8][NL + 1], en[8][NL + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) load_e(j, ec[j]);
    double p[NS];
    int cur = 0;  // offset of the edge row this step writes; the other one holds the previous step's
    for (int base = 0; base < T; base += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) load_e(base + 8 + j, en[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int step = base + j;
            if (step < T) {
                double v[NS];
                if (step == 0) {
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const int st = s0 + i;
                        const bool init = DIR == 0 ? st <= 1 : st >= S - 2;
                        const float e = (i & 1) ? ec[0][i >> 1] : ec[0][NL];
                        v[i] = (live[i] && init) ? (double)e * LOG2E_D : NEG_INF;
                    }
                } else {
                    // LDS-only barrier: __syncthreads() would also drain vmcnt(0) every frame
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    const double* prev = edge + (bstride - cur);
                    double x[NS + 2];  // the previous row around this thread's states: x[OFF + i] = state s0 + i
                    if (DIR == 0) {
                        x[0] = NEG_INF;  // (state s0 - 2: never read, s0 is a blank)
                        x[1] = prev[tid];
                    } else {
                        x[NS] = prev[(tid + 2) * 2];
                        x[NS + 1] = prev[(tid + 2) * 2 + 1];
                    }
#pragma unroll
                    for (int i = 0; i < NS; ++i) x[OFF + i] = p[i];
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        double l;
                        float e;
                        if (i & 1) {
                            e = ec[j][i >> 1];
                            l = lse3_long(x[OFF + i], x[OFF + i + NB], skip[i >> 1] ? x[OFF + i + 2 * NB] : NEG_INF);
                        } else {
                            e = ec[j][NL];
                            l = lse2_long(x[OFF + i], x[OFF + i + NB]);
                        }
                        v[i] = live[i] ? fma((double)e, LOG2E_D, l) : NEG_INF;
                    }
                }
                if (DIR == 0) {
                    edge[cur + tid + 1] = v[NS - 1];
                } else {
                    edge[cur + (tid + 1) * 2] = v[0];
                    edge[cur + (tid + 1) * 2 + 1] = v[1];
                }
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    outp[i] = v[i];
                    p[i] = v[i];
                }
                outp += row_inc;
                cur = bstride - cur;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i <= NL; ++i) {
                asm volatile("" : "+v"(en[j][i]));  // materialise the prefetched chunk here, inside the iteration
                ec[j][i] = en[j][i];
            }
    }
    if (DIR == 0) {  // the last row's two final states, for the loss
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (s0 + i == S - 1) fin[0] = p[i];
            if (s0 + i == S - 2) fin[1] = p[i];
        }
    }
}

template <int NS>
__global__ __launch_bounds__(LONG_THREADS_MAX) void ctc_long_lattice_kernel(
    const float* __restrict__ logq, const int32_t* __restrict__ labels, const int32_t* __restrict__ label_len,
    const int32_t* __restrict__ input_len, double* __restrict__ alpha, double* __restrict__ beta, float* __restrict__ loss,
    float* __restrict__ logz2, int32_t* __restrict__ zint, int32_t* __restrict__ cls, double* __restrict__ dump, int t_out, int k,
    int l_max, int sp, int blank) {
    extern __shared__ double lds_d[];  // recursion: fin[2] | edge rows 2 x (threads + 2) x {1, 2}; list builder: l_max + k + 1 ints
    const int b = blockIdx.x;
    const int dir = blockIdx.y;
    const int tid = threadIdx.x;
    const int L = min(max(label_len[b], 0), l_max);  // (a length outside the label batch must not index outside it)
    const int32_t* lab = labels + (long)b * l_max;
    if (dir == 2) {
        // per-class position lists of this utterance's label for the gradient kernel (counting sort; inside a class the
        // positions stay in label order, which fixes the summation order).  cls[b] = pos[l_max] | start[k + 1], as in ctc.hip.
        int* s_lab = (int*)lds_d;
        int* s_start = s_lab + l_max;
        int32_t* pos_out = cls + (long)b * (l_max + k + 1);
        int32_t* start_out = pos_out + l_max;
        const int nt = blockDim.x;
        for (int i = tid; i < L; i += nt) s_lab[i] = lab[i];
        for (int i = tid; i <= k; i += nt) s_start[i] = 0;
        __syncthreads();
        // rank of position i inside its class = number of earlier positions with the same letter.  The work-group has at
        // least S / NS > L / 2 threads: at most 2 positions per thread (registers, indexed by unrolled constants).
        int ranks[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * nt;
            if (i < L) {
                const int c = s_lab[i];
                int r = 0;
                for (int j = 0; j < i; ++j) r += (s_lab[j] == c);
                ranks[u] = r;
                atomicAdd(&s_start[c + 1], 1);  // integer count: order-independent
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int c = 0; c < k; ++c) s_start[c + 1] += s_start[c];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + u * nt;
            if (i < L) pos_out[s_start[s_lab[i]] + ranks[u]] = i;
        }
        for (int i = tid; i <= k; i += nt) start_out[i] = s_start[i];
        return;
    }
    const int S = 2 * L + 1;
    int T = input_len[b];
    if (T > t_out) T = t_out;
    if (T <= 0) {
        if (dir == 0 && tid == 0) {
            loss[b] = INFINITY;
            zint[b] = 0;
            logz2[b] = -INFINITY;
        }
        return;
    }
    double* fin = lds_d;
    double* edge = lds_d + 2;
    const float* lq_b = logq + (long)b * t_out * k;
    const long lat = (long)b * t_out * sp;
    double* dump_b = dump + ((long)b * 2 + dir) * LONG_DUMP_DOUBLES;
    if (dir == 0)
        long_lattice_run<NS, 0>(lq_b, lab, L, S, T, k, blank, sp, alpha + lat, dump_b, edge, fin);
    else
        long_lattice_run<NS, 1>(lq_b, lab, L, S, T, k, blank, sp, beta + lat, dump_b, edge, fin);
    if (dir == 0) {
        __syncthreads();
        if (tid == 0) {
            // loss, and log2 Z for the gradient pass with integer part and fraction apart (as repair_lattices hands them over)
            const double last = fin[0], last2 = fin[1];
            const double m = fmax(last, last2);
            const double lp2 = (m == NEG_INF) ? NEG_INF : m + log2(exp2(last - m) + exp2(last2 - m));
            loss[b] = (float)(-lp2 * LN2_D);
            const double fl = (m == NEG_INF) ? 0.0 : floor(lp2);
            zint[b] = (int32_t)fl;
            logz2[b] = (m == NEG_INF) ? -INFINITY : (float)(lp2 - fl);
        }
    }
}

// One wave per frame; work-group = 4 waves x frames_per_wg / 4 frames of one utterance.  The frame's alpha and beta rows are
// read in chunks of 64 columns, four chunks' loads in flight; alpha + beta - floor(log2 Z) in doubles, the small rest in fp32.
// LDS: labels[l_max] | class_pos[l_max] | class_start[k + 1] | lq[4][64] | gamma[4][l_max]  (50.4 KB at l_max = 2047)
__global__ __launch_bounds__(256) void ctc_long_grad_kernel(
    const float* __restrict__ probs, const float* __restrict__ logq, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ label_len, const int32_t* __restrict__ input_len, const double* __restrict__ alpha,
    const double* __restrict__ beta, const float* __restrict__ logz2, const int32_t* __restrict__ zint,
    const float* __restrict__ loss, const int32_t* __restrict__ cls, void* __restrict__ dlogits, int t_out, int k, int l_max,
    int sp, int blank, int frames_per_wg, int g_row0, int g_rs, long g_bs, int out_f32, float eps, float grad_scale) {
    extern __shared__ int lds_i[];
    int* s_lab = lds_i;
    int* s_pos = s_lab + l_max;
    int* s_start = s_pos + l_max;
    float* s_lq = (float*)(s_start + (k + 1));
    float* s_gam = s_lq + 4 * 64;
    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int L = min(max(label_len[b], 0), l_max);  // (a length outside the label batch must not index outside it)
    const int S = 2 * L + 1;
    int T = input_len[b];
    if (T > t_out) T = t_out;
    const int32_t* lab = labels + (long)b * l_max;
    const int32_t* cpos = cls + (long)b * (l_max + k + 1);
    for (int i = tid; i < L; i += 256) {
        s_lab[i] = lab[i];
        s_pos[i] = cpos[i];
    }
    if (tid <= k) s_start[tid] = cpos[l_max + tid];
    __syncthreads();
    const bool feasible = loss[b] < INFINITY;
    const float log_p = logz2[b];  // the fraction of log2 Z
    const double zi = (double)zint[b];
    const int nj = (S + 63) >> 6;  // chunks that hold live states (the rest of the row is -inf padding)
    float* gam = s_gam + wave * l_max;
    float* wlq = s_lq + wave * 64;
    const int t_begin = blockIdx.x * frames_per_wg;
    for (int tt = wave; tt < frames_per_wg; tt += 4) {
        const int t = t_begin + tt;
        if (t >= t_out) break;
        const long fidx = (long)b * t_out + t;
        float dz = 0.f;
        if (t < T) {
            const float lqv = lane < k ? logq[fidx * k + lane] : 0.f;
            const float pk = lane < k ? probs[fidx * k + lane] : 0.f;
            float occ = 0.f;
            if (feasible) {
                const double* al = alpha + fidx * sp + lane;
                const double* be = beta + fidx * sp + lane;
                wlq[lane] = lqv * LOG2E;  // emission in lattice units: log2 q
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const float lq_blank = wlq[blank];
                // blank states (even s) -> butterfly sum; letter states (odd s) -> gamma[] in LDS
                float blank_part = 0.f;
                for (int j0 = 0; j0 < nj; j0 += 4) {
                    double ad[4], bd[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {  // (wave-uniform bound; nj * 64 <= sp)
                        const bool in = j0 + u < nj;
                        ad[u] = in ? al[64 * (j0 + u)] : NEG_INF;
                        bd[u] = in ? be[64 * (j0 + u)] : NEG_INF;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int s = lane + 64 * (j0 + u);
                        if (s < S) {
                            const float ab = (ad[u] == NEG_INF || bd[u] == NEG_INF) ? -INFINITY : (float)((ad[u] + bd[u]) - zi);
                            if (s & 1) {
                                const int pos = s >> 1;
                                const float lg = ab - wlq[s_lab[pos]] - log_p;
                                gam[pos] = (ab == -INFINITY) ? 0.f : exp2f(lg);
                            } else {
                                const float lg = ab - lq_blank - log_p;
                                blank_part += (ab == -INFINITY) ? 0.f : exp2f(lg);
                            }
                        }
                    }
                }
                blank_part = wave_sum(blank_part);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (lane < k) {
                    if (lane == blank) {
                        occ = blank_part;
                    } else {
                        const int e0 = s_start[lane], e1 = s_start[lane + 1];
                        for (int i = e0; i < e1; ++i) occ += gam[s_pos[i]];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            // du_k = q_k - occ_k ; dp_k = du_k / (p_k + eps) ; dz_k = p_k * (dp_k - sum_j p_j dp_j)
            float dp = 0.f;
            if (lane < k) dp = (expf(lqv) - occ) / (pk + eps);
            const float inner = wave_sum(pk * dp);
            dz = pk * (dp - inner) * grad_scale;
        }
        if (lane < k) {
            const long gi = (long)b * g_bs + (long)(g_row0 + t) * g_rs + lane;
            if (out_f32)
                ((float*)dlogits)[gi] = dz;
            else
                ((unsigned short*)dlogits)[gi] = f32_to_bf16_bits(dz);
        }
    }
}

}  // namespace

size_t ctc_long_dump_bytes(int batch) { return (size_t)batch * 2 * LONG_DUMP_DOUBLES * sizeof(double); }

int ctc_long_loss_grad(const float* probs, const float* logq, const int32_t* labels, const int32_t* label_len,
                       const int32_t* input_len, float* loss, void* dlogits, int batch, int t_out, int k, int l_max, int g_row0,
                       int g_row_stride, long g_batch_stride, int out_f32, float eps, float grad_scale, double* alpha,
                       double* beta, int32_t* cls, float* logz2, int32_t* zint, double* dump, hipStream_t s) {
    const int sp = lattice_sp(l_max);
    const int ns = sp <= 2 * LONG_THREADS_MAX ? 2 : 4;  // l_max <= 1023: two states per thread
    if (sp > 4 * LONG_THREADS_MAX) {
        sl_set_error("ctc_long_loss_grad: l_max %d > %d", l_max, SL_CTC_MAX_LABEL);
        return SL_ERR_UNSUPPORTED;
    }
    const int threads = (sp / ns + 63) / 64 * 64;  // whole waves that cover the row; dead lanes only in the last one
    size_t lds = (size_t)(2 + 2 * (threads + 2) * 2) * sizeof(double);
    const size_t lds_lists = (size_t)(l_max + k + 1) * sizeof(int);
    if (lds < lds_lists) lds = lds_lists;
    if (ns == 2)
        hipLaunchKernelGGL(ctc_long_lattice_kernel<2>, dim3(batch, 3), dim3(threads), lds, s, logq, labels, label_len, input_len,
                           alpha, beta, loss, logz2, zint, cls, dump, t_out, k, l_max, sp, k - 1);
    else
        hipLaunchKernelGGL(ctc_long_lattice_kernel<4>, dim3(batch, 3), dim3(threads), lds, s, logq, labels, label_len, input_len,
                           alpha, beta, loss, logz2, zint, cls, dump, t_out, k, l_max, sp, k - 1);
    int rc = sl_check_launch("sl_ctc_loss_grad(long lattice)");
    if (rc != SL_OK) return rc;
    const int frames_per_wg = 8;  // two frames per wave, as ctc_grad_kernel
    const size_t lds2 = (size_t)(2 * l_max + (k + 1)) * sizeof(int) + (size_t)(4 * 64 + 4 * l_max) * sizeof(float);
    const dim3 grid((t_out + frames_per_wg - 1) / frames_per_wg, batch);
    hipLaunchKernelGGL(ctc_long_grad_kernel, grid, dim3(256), lds2, s, probs, logq, labels, label_len, input_len,
                       (const double*)alpha, (const double*)beta, (const float*)logz2, (const int32_t*)zint, (const float*)loss, cls,
                       dlogits, t_out, k, l_max, sp, k - 1, frames_per_wg, g_row0, g_row_stride, g_batch_stride, out_f32, eps,
                       grad_scale);
    return sl_check_launch("sl_ctc_loss_grad(long grad)");
}
