// asg_beam.hip -- ASG beam search (a max search over prefixes under emissions + transition scores), with or without the
// n-gram scorer, for gfx950.  No reference counterpart (the reference has no ASG: speechless/net.py:397-399); the definition,
// bit for bit in fp32, is include/speechless_hip.h at sl_asg_beam_search.  DESIGN.md section 3.5 explains the shape.
//
// Kernel asg_beam_kernel: ONE WORK-GROUP of four waves per utterance.  The beam is an ordered list of n <= W positions in LDS
// (position -> storage, score, last grapheme, node id); a storage holds a prefix's scorer state and, with a language model,
// the scorer's score behind each of its k children (cache[e][j]: behind character j; columns k-2 and k-1: behind the last
// character written once and twice more, which the two repeat marks use; a delta is the difference of two of them).  Per frame:
//   1. candidates: wave w takes the positions w, w+4, ..; lane = grapheme j computes a(i, j) from s_i, the LDS-resident row
//      g(l_i, .) and the staged emissions, one rounded operation per line of the definition, into cand[i * 64 + j];
//   2. merge: a position whose parent prefix is in the beam (found by node id) names the same prefix as the parent's
//      extension by its last grapheme: the later of the two in candidate order becomes -inf;
//   3. exact top-W: a radix select over ord(score), 8 bits a pass, LDS histograms summed from the top by wave 0; the
//      survivors above the threshold and the first ones AT it in index order ((i, j) ascending = the index) are compacted
//      and rank-sorted by (score descending, index ascending).  No insertion loop: the frame's result is a function of the
//      candidate set alone;
//   4. the new beam: a stay or a merged extension keeps its prefix's storage; a new prefix gets its canonical node id from
//      the per-utterance hash map (parent node, label) -> node in the workspace (so a prefix that left the beam and comes
//      back is the same node), its scorer state from the parent's state and cache (a trie step or a history shift), a free storage
//      and -- with a language model -- its children's scores from the trie and n-gram tables in HBM (the only dependent
//      global loads of a frame).
// The storages' common fields, the node table, the scorer and the backtrace are beam_shared.h's.
// Frames are staged in LDS CH at a time; the K x K transition scores and the start scores stay in LDS for the whole utterance.
// The kernel uses no scratch (build.py NO_SCRATCH) and no float atomics; the only multiply is lm_weight * delta, rounded
// before its add (-ffp-contract=off).
#include "beam_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;  // threads of the work-group
constexpr uint32_t ORD_NEG_INF = 0x007FFFFFu;  // ord(-inf)

enum { C_NS, C_NNEW, C_NODES, C_ALL, C_PREFIX, C_NEED, C_EQ, C_OVER, C_TOP, C_COUNT, C_N };

struct Lds : BeamStorages {  // cache[e][j]: the scorer's score behind each child of storage e, [k-2], [k-1]: see the head
    float cand[WMAX * KMAX];       // this frame's candidates, index i * 64 + j (the end: the totals)
    float g[(KMAX + 1) * KMAX];    // g[l * 64 + j]; row k: the start scores (the root's "last grapheme" is k)
    float frames[CH][KMAX];
    uint8_t cbt[WMAX * KMAX];      // candidate index of a winning merged extension -> the position it names, 0xFF
    int bins[4][256];              // the radix select's histograms, one per pass
    // per beam position
    int b_e[WMAX], b_l[WMAX], b_node[WMAX], b_ext[WMAX];
    float b_s[WMAX];
    // survivors of the frame
    unsigned long long skey[WMAX], sorted[WMAX];
    int wtie[4];
    int ctr[C_N];
};
static_assert(sizeof(Lds) == 110392, "the LDS of a work-group: occupancy");

__global__ __launch_bounds__(NT) void asg_beam_kernel(const float* __restrict__ logq, const float* __restrict__ trans,
                                                      const float* __restrict__ init, const int32_t* __restrict__ input_len,
                                                      int t_out, int k, int W, int has_lm, sl_beam_lm lm,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                      float* __restrict__ score, uint8_t* __restrict__ ws, BeamSizes sizes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Lds& S = *(Lds*)smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const NodeTable nodes(ws, b, sizes);
    const int T = max(0, min(input_len[b], t_out));
    const int nchar = k - 2;  // characters; k - 2 = asg_twice, k - 1 = asg_thrice
    const float lw = lm.lm_weight;
    int32_t* row = out + (size_t)b * t_out;

    // ---- tables, the root (storage 0, node 0, "last grapheme" k = none, score -0 so that -0 + g0(j) is g0(j) bit for bit)
    for (int q = tid; q < k * k; q += NT) S.g[(q / k) * KMAX + (q % k)] = trans[q];
    if (tid < k) S.g[k * KMAX + tid] = init[tid];
    for (int q = tid; q < WMAX * KMAX / 4; q += NT) ((uint32_t*)S.cbt)[q] = 0xFFFFFFFFu;
    if (tid == 0) {
        init_root(S, nodes.arena, k, lm.bos);
        S.b_e[0] = 0;
        S.b_l[0] = k;
        S.b_node[0] = 0;
        S.b_ext[0] = -1;
        S.b_s[0] = -0.f;
        S.ctr[C_NODES] = 1;
        S.ctr[C_OVER] = 0;
    }
    __syncthreads();

    // scorer scores of the children of the storages freelist[0 .. n_new)
    auto fill_cache = [&](int n_new) {
        for (int q = tid; q < n_new * k; q += NT) {
            const int r = q / k, m = q - r * k;
            const int e = S.freelist[r];
            const int l = S.label[e];
            St st = load_state(S, e);
            if (m < nchar) {
                expand(lm, nchar, st, m);
                S.cache[e][m] = st.score;
            } else if (l < nchar) {
                expand(lm, nchar, st, l);
                if (m == k - 1) expand(lm, nchar, st, l);
                S.cache[e][m] = st.score;
            }
        }
        __syncthreads();
    };
    if (has_lm) fill_cache(1);

    int n = 1;  // beam size
    for (int t = 0; t < T && n > 0; ++t) {
        const int f0 = t % CH;
        if (f0 == 0) {
            const int nf = min(CH, T - t);
            const float* src = logq + ((size_t)b * t_out + t) * k;
            for (int q = tid; q < nf * k; q += NT) S.frames[q / k][q % k] = src[q];
        }
        for (int q = tid; q < 4 * 256; q += NT) (&S.bins[0][0])[q] = 0;
        if (tid < WMAX) S.used[tid] = 0;
        if (tid == 0) S.ctr[C_NS] = S.ctr[C_NNEW] = S.ctr[C_ALL] = 0;
        __syncthreads();
        const float* em = S.frames[f0];
        const int N = n * KMAX;

        // ---- 1. candidates
        for (int i = wave; i < n; i += NT / 64) {
            const int l = S.b_l[i], e = S.b_e[i];
            const float s = S.b_s[i];
            float a = NEG_INF;
            if (lane < k) {
                a = s + S.g[l * KMAX + lane];
                a = a + em[lane];
                if (has_lm && lane != l) {  // delta = the scorer's score behind a character - the one before it
                    if (lane < nchar) {
                        a = lw * (S.cache[e][lane] - S.score[e]) + a;
                    } else if (l < nchar) {
                        const float once = S.cache[e][k - 2];
                        a = lw * (once - S.score[e]) + a;
                        if (lane == k - 1) a = lw * (S.cache[e][k - 1] - once) + a;
                    }
                }
                if (!(a > NEG_INF)) a = NEG_INF;
            }
            S.cand[i * KMAX + lane] = a;
        }
        __syncthreads();

        // ---- 2. merge: the stay of position i and its parent's extension by l_i name the same prefix
        if (tid < n) {
            const int i = tid, l = S.b_l[i];
            const int pn = S.pnode[S.b_e[i]];
            int pp = -1;
            for (int q = 0; q < n; ++q) pp = S.b_node[q] == pn ? q : pp;
            int ext = -1;
            if (pn >= 0 && pp >= 0) {
                const int ie = pp * KMAX + l, is = i * KMAX + l;
                const float ve = S.cand[ie], vs = S.cand[is];
                if (ve > vs || (ve == vs && pp < i)) {
                    S.cand[is] = NEG_INF;
                    if (ve > NEG_INF) {
                        S.cbt[ie] = (uint8_t)i;
                        ext = ie;
                    }
                } else {
                    S.cand[ie] = NEG_INF;
                }
            }
            S.b_ext[i] = ext;
        }
        __syncthreads();

        // ---- 3. exact top-W: radix select of the W-th largest ord(score), then the ties in index order
        uint32_t prefix = 0;
        int need = W, eq = 0;
        bool all = false;
        for (int p = 0; p < 4; ++p) {
            const int shift = 24 - 8 * p;
            int cur = 0, cnt = 0;  // (scores cluster in a few bins of the high bytes: a thread adds a run of one bin at once)
            for (int idx = tid; idx < N; idx += NT) {
                const float c = S.cand[idx];
                if (c > NEG_INF) {
                    const uint32_t o = ord(c);
                    if (p == 0 || (o >> (shift + 8)) == prefix) {
                        const int bin = (int)((o >> shift) & 255u);
                        if (bin != cur && cnt) {
                            atomicAdd(&S.bins[p][cur], cnt);
                            cnt = 0;
                        }
                        cur = bin;
                        ++cnt;
                    }
                }
            }
            if (cnt) atomicAdd(&S.bins[p][cur], cnt);
            __syncthreads();
            if (wave == 0) {
                int c[4], tot = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = S.bins[p][255 - 4 * lane - q];
                    tot += c[q];
                }
                int incl = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int v = __shfl_up(incl, off);
                    if (lane >= off) incl += v;
                }
                const int total = __shfl(incl, 63);
                int run = incl - tot;
                if (p == 0 && total <= need) {
                    if (lane == 0) S.ctr[C_ALL] = 1;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (run < need && run + c[q] >= need) {
                            S.ctr[C_PREFIX] = (int)((prefix << 8) | (uint32_t)(255 - 4 * lane - q));
                            S.ctr[C_NEED] = need - run;
                            S.ctr[C_EQ] = c[q];
                        }
                        run += c[q];
                    }
                }
            }
            __syncthreads();
            all = S.ctr[C_ALL] != 0;
            if (all) break;
            prefix = (uint32_t)S.ctr[C_PREFIX];
            need = S.ctr[C_NEED];
            eq = S.ctr[C_EQ];
        }
        const uint32_t thr = all ? ORD_NEG_INF : prefix;  // survivors: ord > thr, and `need` of the eq candidates AT thr
        const bool ties = !all && eq > need;
        for (int idx = tid; idx < N; idx += NT) {
            const float c = S.cand[idx];
            if (c > NEG_INF) {
                const uint32_t o = ord(c);
                if (o > thr || (o == thr && !all && !ties)) {
                    const int pos = atomicAdd(&S.ctr[C_NS], 1);
                    if (pos < WMAX) S.skey[pos] = ((unsigned long long)~o << 32) | (uint32_t)idx;
                }
            }
        }
        if (ties) {  // more candidates at the threshold than places: the first `need` in index order (wave w: its quarter)
            const int q0 = wave * (N / 4), q1 = q0 + N / 4;
            int cnt = 0;
            for (int base = q0; base < q1; base += 64) {
                const int idx = base + lane;
                const float c = idx < q1 ? S.cand[idx] : NEG_INF;
                cnt += __popcll(__ballot(c > NEG_INF && ord(c) == thr));
            }
            if (lane == 0) S.wtie[wave] = cnt;
            __syncthreads();
            int run = 0;
            for (int w = 0; w < wave; ++w) run += S.wtie[w];
            for (int base = q0; base < q1 && run < need; base += 64) {
                const int idx = base + lane;
                const float c = idx < q1 ? S.cand[idx] : NEG_INF;
                const bool tie = c > NEG_INF && ord(c) == thr;
                const uint64_t m = __ballot(tie);
                if (tie && run + lanes_below(m) < need) {
                    const int pos = atomicAdd(&S.ctr[C_NS], 1);
                    if (pos < WMAX) S.skey[pos] = ((unsigned long long)~thr << 32) | (uint32_t)idx;
                }
                run += __popcll(m);
            }
        }
        __syncthreads();
        const int ns = min(S.ctr[C_NS], W);
        if (tid < ns) {
            const unsigned long long key = S.skey[tid];
            int rank = 0;
            for (int q = 0; q < ns; ++q) rank += S.skey[q] < key;
            S.sorted[rank] = key;
        }
        __syncthreads();

        // ---- 4. the new beam.  phase A: read what a position needs (its parent's storage may be recycled below)
        int my_e = -1, my_node = 0, my_pn = 0, my_l = 0, my_q = 0;
        float my_a = NEG_INF;
        St st = {};
        if (tid < ns) {
            const int idx = (int)(uint32_t)S.sorted[tid];
            const int i = idx >> 6, j = idx & 63;
            const int pe = S.b_e[i], l = S.b_l[i];
            my_a = S.cand[idx];
            my_l = j;
            const int m = S.cbt[idx];
            if (j == l) {
                my_e = pe;
            } else if (m != 0xFF) {
                my_e = S.b_e[m];
            }
            if (my_e >= 0) {
                S.used[my_e] = 1;
                my_node = S.node[my_e];
            } else {
                my_q = atomicAdd(&S.ctr[C_NNEW], 1);
                my_pn = S.node[pe];
                st = load_state(S, pe);
                if (has_lm && (j < nchar || l < nchar)) {
                    // the state behind the characters grapheme j writes behind l (j, or l once / twice): its score is the
                    // parent's cache[j]
                    const int c = j < nchar ? j : l;
                    const int reps = j == k - 1 ? 2 : 1;
                    const float behind = S.cache[pe][j];
                    for (int r = 0; r < reps; ++r) step_into_child(lm, nchar, st, c, behind);
                }
                // canonical node id of (parent node, label): the hash map, or a fresh node (an LDS counter: the threads
                // that need one are any subset of the work-group)
                const uint32_t key = node_key(my_pn, j);
                uint64_t slot;
                int found = nodes.find(key, slot);
                if (found < 0) {
                    const int id = atomicAdd(&S.ctr[C_NODES], 1);
                    if (id < nodes.node_cap) {
                        nodes.insert(slot, key, id, my_pn, j);
                        found = id;
                    } else {
                        S.ctr[C_OVER] = 1;
                        found = 0;
                    }
                }
                my_node = found;
            }
        }
        __syncthreads();
        const int n_new = S.ctr[C_NNEW];
        if (wave == 0) build_freelist(S.used, W, S.freelist, lane);  // the storages no survivor holds
        if (tid < n && S.b_ext[tid] >= 0) S.cbt[S.b_ext[tid]] = 0xFF;
        __syncthreads();
        // phase B: the positions of the new beam, the new prefixes into free storages
        if (tid < ns) {
            if (my_e < 0) {
                my_e = S.freelist[my_q];
                S.node[my_e] = my_node;
                S.pnode[my_e] = my_pn;
                S.label[my_e] = my_l;
                store_state(S, my_e, st);
            }
            S.b_e[tid] = my_e;
            S.b_l[tid] = my_l;
            S.b_node[tid] = my_node;
            S.b_s[tid] = my_a;
        }
        n = ns;
        __syncthreads();
        if (has_lm && n_new > 0) fill_cache(n_new);
    }

    // ---- end of utterance: expand_state_end, the first maximal total in beam order, the backtrace
    if (T == 0) n = 0;
    if (tid < n) {
        float total = S.b_s[tid];
        if (has_lm) total = lw * expand_end_delta(lm, load_state(S, S.b_e[tid])) + total;
        S.cand[tid] = total;
    }
    __syncthreads();
    if (tid == 0) {
        int top = -1, count = 0;
        float best = NEG_INF;
        for (int i = 0; i < n; ++i) {
            const float v = S.cand[i];
            if (top < 0 || v > best) {
                top = i;
                best = v;
            }
        }
        if (top >= 0) count = count_labels(nodes.arena, S.b_node[top], T, false);
        S.ctr[C_TOP] = top;
        S.ctr[C_COUNT] = count;
        if (score) score[b] = best;
    }
    __syncthreads();
    const int count = min(S.ctr[C_COUNT], t_out);
    for (int i = count + tid; i < t_out; i += NT) row[i] = -1;
    if (tid == 0) {
        if (S.ctr[C_TOP] >= 0) write_labels(nodes.arena, S.b_node[S.ctr[C_TOP]], T, false, row, S.ctr[C_COUNT], t_out);
        out_len[b] = S.ctr[C_OVER] ? -1 : count;
    }
}

}  // namespace

extern "C" size_t sl_asg_beam_search_workspace_bytes(int batch, int t_out, int k, int beam_width) {
    return beam_workspace_bytes(batch, t_out, k, beam_width);
}

extern "C" int sl_asg_beam_search(const float* logq, const float* trans, const float* init, const int32_t* input_len, int batch,
                                  int t_out, int k, int beam_width, const sl_beam_lm* lm, int32_t* out, int32_t* out_len,
                                  float* score, void* workspace, size_t workspace_bytes, void* stream) {
    static const BeamWords words = {"sl_asg_beam_search", "t_out", "grapheme", "characters"};
    SL_CHECK_ARG(logq && trans && init && input_len && out && out_len && workspace, "sl_asg_beam_search: null pointer");
    const int rc = beam_check_args(words, batch, t_out, k, beam_width, lm, k - 2);
    if (rc != SL_OK) return rc;
    SL_CHECK_ARG(!lm || k > 2, "sl_asg_beam_search: a language model needs at least one character beside the two repeat marks");
    const hipStream_t s = (hipStream_t)stream;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)asg_beam_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds));
        attr_set = true;
    }
    const int ws_rc = beam_clear_workspace(words.fn, workspace, workspace_bytes,
                                           beam_workspace_bytes(batch, t_out, k, beam_width), s);
    if (ws_rc != SL_OK) return ws_rc;
    hipLaunchKernelGGL(asg_beam_kernel, dim3(batch), dim3(NT), sizeof(Lds), s, logq, trans, init, input_len, t_out, k,
                       beam_width, lm ? 1 : 0, lm ? *lm : beam_lm_none(), out, out_len, score, (uint8_t*)workspace,
                       beam_sizes_of(t_out, beam_width));
    return sl_check_launch(words.fn);
}
