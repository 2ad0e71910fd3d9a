// ctc_beam.hip -- CTC prefix beam search, with or without the n-gram scorer, for gfx950.
//
// The device twin of csrc_host/beam_search.cpp (TensorFlow 1.x's CTCBeamSearchDecoder + the KenLM-style scorer).
// Semantics and tolerances: include/speechless_hip.h, sl_ctc_beam_search.  DESIGN.md section 3.3 explains the shape.
//
// Kernel ctc_beam_kernel: ONE WAVE per utterance.  The beam lives in LDS as W "storages" (one per beam entry: node id,
// probabilities, scorer state and, with a language model, the scores of all k-1 children of the entry) and a list of
// W slots in the host's slot order (slot -> storage), so that eviction ("the first minimum in slot order") and the
// tie rules are the host's.  Per frame:
//   1. stable rank sort of the slots by total (descending) = the host's `branches`;
//   2. the first loop for all branches at once (a branch only reads its parent's OLD probabilities; the parent-active
//      test is exact for finite inputs, and a wave-uniform sequential pass redoes the frame when an input of -inf makes
//      a parent's activity change within the loop);
//   3. the child loop, branch by branch in sorted order: lane = label computes all k-1 child totals in parallel, and
//      only the children that can change the beam -- total above the current bottom, or a child that is itself a
//      branch of this frame -- go through the host's sequential is_candidate / evict-first-minimum / push step, in
//      label order, with a wave reduction for the new bottom after each insertion;
//   4. the new entries get their canonical node ids from a per-utterance hash map (parent node, label) -> node in the
//      workspace (next to the node arena the backtrace walks), their scorer state, and -- with a language model -- their
//      children's scores from the flat trie and n-gram tables in HBM (the only dependent global loads of a frame).
// Frames are staged in LDS CH at a time and normalised there (log(p + eps) - logsumexp, the host's operation order).
// The kernel uses no scratch (build.py NO_SCRATCH): every per-lane array is indexed with compile-time indices.
// From beam_shared.h it takes the limits, the n-gram look-up, advance, trie_word, ord / unord, the workspace layout and the
// host-side checks.  Its storages, its hash-map look-up and insert, its backtrace and its scorer arithmetic (fill_cache, phase
// A of step 4, the end of the utterance) are still written out here, in the operation order that beam_shared.h states at
// expand(): moving this kernel onto the header's BeamStorages / NodeTable / St cost it 1 % of its time.
#include "beam_shared.h"

#pragma clang fp contract(off)  // lm_weight * delta + previous is two roundings on the host

namespace {

__device__ __forceinline__ float log_d(float x) { return (float)log((double)x); }
__device__ __forceinline__ float exp_d(float x) { return (float)exp((double)x); }

// beam_search.cpp log_sum_exp
__device__ __forceinline__ float lse(float a, float b) {
    if (a == NEG_INF) return b;
    if (b == NEG_INF) return a;
    return a > b ? a + (float)log1p((double)exp_d(b - a)) : b + (float)log1p((double)exp_d(a - b));
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

struct Lds {
    float frames[CH][KMAX + 1];
    float norm[CH];
    // per storage
    int node[WMAX], pnode[WMAX], label[WMAX], trie[WMAX], hlen[WMAX];
    float nt[WMAX], nb[WMAX], nl[WMAX], lm[WMAX], score[WMAX], delta[WMAX];
    uint32_t hist[HMAX][WMAX];
    float cache[WMAX][KMAX];  // with a language model: the `score` of each child (its delta = cache - score)
    // per branch position (this frame's sorted order)
    int b_e[WMAX], b_node[WMAX], b_ppos[WMAX], b_slot[WMAX], b_reset[WMAX];
    float b_ot[WMAX], b_ob[WMAX], b_onl[WMAX];
    // per slot
    int slot_e[WMAX], slot_src[WMAX];
    float slot_tot[WMAX];
    int freelist[WMAX], used[WMAX];
    alignas(16) int8_t cbt[WMAX * KMAX];  // [branch i][label] -> branch j = child(i, label), -1
    int scalar[4];
};

__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ probs, const int32_t* __restrict__ lengths,
                                                      int t_max, int k, int blank, int W, int merge, float eps, int has_lm,
                                                      sl_beam_lm lm, int32_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                      float* __restrict__ log_prob, uint8_t* __restrict__ ws, int64_t node_cap,
                                                      int64_t hash_slots, int64_t ws_stride) {
    __shared__ Lds S;
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    int32_t* arena = (int32_t*)(ws + (size_t)b * ws_stride);
    unsigned long long* hmap = (unsigned long long*)(ws + (size_t)b * ws_stride + (((size_t)node_cap * 4 + 7) & ~(size_t)7));
    const uint64_t hmask = (uint64_t)hash_slots - 1;
    const int len = max(0, min(lengths[b], t_max));
    const int nlab = k - 1;  // alphabet size (blank = k - 1 when has_lm)
    const float lw = lm.lm_weight;

    // ---- root (storage 0, node 0)
    int size = 1;
    int64_t n_nodes = 1;
    bool overflow = false;
    if (lane == 0) {
        arena[0] = -1;
        S.node[0] = 0;
        S.pnode[0] = -1;
        S.label[0] = -1;
        S.nt[0] = 0.f;
        S.nb[0] = 0.f;
        S.nl[0] = NEG_INF;
        S.lm[0] = S.score[0] = S.delta[0] = 0.f;
        S.trie[0] = 0;
        S.hlen[0] = 1;
        for (int j = 0; j < HMAX; ++j) S.hist[j][0] = j == HMAX - 1 ? (uint32_t)lm.bos : 0u;
        S.slot_e[0] = 0;
        S.freelist[0] = 0;
    }
    __syncthreads();

    // children scores of the storages freelist[0 .. n_new): the scorer's expand_state for every label
    auto fill_cache = [&](int n_new) {
        for (int r = lane; r < n_new; r += 64) {
            const int e = S.freelist[r];
            if (lm.space_label >= 0) {
                uint32_t h[HMAX];
#pragma unroll
                for (int j = 0; j < HMAX; ++j) h[j] = S.hist[j][e];
                const uint32_t word = (uint32_t)trie_word(lm, S.trie[e]);
                const float d = ngram_score(lm, h, S.hlen[e], word);
                float v = S.lm[e];
                if (word != 0u) v += lm.valid_word_count_weight;
                v += lm.word_count_weight;
                S.cache[e][lm.space_label] = v + d;
            }
        }
        for (int q = lane; q < n_new * nlab; q += 64) {
            const int r = q / nlab, m = q - r * nlab;
            if (m == lm.space_label) continue;
            const int e = S.freelist[r];
            const int tr = S.trie[e];
            const float mu = tr >= 0 && tr < lm.n_trie_nodes ? lm.trie_min[(size_t)tr * nlab + m] : lm.oov_score;
            S.cache[e][m] = mu + S.lm[e];
        }
        __syncthreads();
    };
    if (has_lm) fill_cache(1);

    for (int t = 0; t < len; ++t) {
        // ---- stage and normalise CH frames (beam_search.cpp decode_range)
        const int f0 = t % CH;
        if (f0 == 0) {
            const int nf = min(CH, len - t);
            const float* src = probs + ((size_t)b * t_max + t) * k;
            for (int q = lane; q < nf * k; q += 64) {
                const int f = q / k, j = q - f * k;
                S.frames[f][j] = log_d(src[q] + eps);
            }
            __syncthreads();
            if (lane < nf) {
                float mx = NEG_INF;
                for (int j = 0; j < k; ++j) mx = mx < S.frames[lane][j] ? S.frames[lane][j] : mx;
                float sum = 0.f;
                for (int j = 0; j < k; ++j) sum += exp_d(S.frames[lane][j] - mx);
                S.norm[lane] = mx + log_d(sum);
            }
            __syncthreads();
            for (int q = lane; q < nf * k; q += 64) {
                const int f = q / k, j = q - f * k;
                S.frames[f][j] -= S.norm[f];
            }
            __syncthreads();
        }
        const float* in = S.frames[f0];
        const int n = size;  // branches

        // ---- 1. stable sort of the slots by total, descending
        for (int s = lane; s < n; s += 64) S.slot_tot[s] = S.nt[S.slot_e[s]];
        __syncthreads();
        for (int s = lane; s < n; s += 64) {
            const float v = S.slot_tot[s];
            int rank = 0;
            for (int q = 0; q < n; ++q) {
                const float u = S.slot_tot[q];
                rank += (u > v) || (u == v && q < s);
            }
            const int e = S.slot_e[s];
            S.b_e[rank] = e;
            S.b_node[rank] = S.node[e];
            S.b_ot[rank] = S.nt[e];
            S.b_ob[rank] = S.nb[e];
            S.b_onl[rank] = S.nl[e];
        }
        __syncthreads();
        for (int p = lane; p < n; p += 64) {
            const int pn = S.pnode[S.b_e[p]];
            int pp = -1;
            for (int q = 0; q < n; ++q) pp = S.b_node[q] == pn ? q : pp;
            S.b_ppos[p] = pn < 0 ? -1 : pp;
            S.b_slot[p] = p;
            S.b_reset[p] = 0;
            S.slot_src[p] = p;
        }
        for (int q = lane; q < WMAX * KMAX / 16; q += 64) ((int4*)S.cbt)[q] = make_int4(-1, -1, -1, -1);
        __syncthreads();

        // ---- 2. first loop (every branch from its parent's old probabilities)
        for (int p = lane; p < n; p += 64) {
            const int e = S.b_e[p];
            float nl = S.b_onl[p];
            if (S.pnode[e] >= 0) {
                const int q = S.b_ppos[p];
                if (q >= 0 && S.b_ot[q] != NEG_INF) {
                    const float prev = (merge && S.label[e] == S.label[S.b_e[q]]) ? S.b_ob[q] : S.b_ot[q];
                    nl = lse(nl, has_lm ? lw * S.delta[e] + prev : prev);
                }
                nl = nl + in[S.label[e]];
            }
            const float nb = S.b_ot[p] + in[blank];
            S.nl[e] = nl;
            S.nb[e] = nb;
            S.nt[e] = lse(nb, nl);
            const int q = S.b_ppos[p];
            if (q >= 0) S.cbt[q * KMAX + S.label[e]] = (int8_t)p;
        }
        __syncthreads();
        {
            bool odd = false;
            for (int p = lane; p < n; p += 64) {
                const int q = S.b_ppos[p];
                odd |= q >= 0 && q < p && ((S.nt[S.b_e[q]] == NEG_INF) != (S.b_ot[q] == NEG_INF));
            }
            if (__ballot(odd)) {  // a parent's activity changed inside the loop: the host's order, one branch at a time
                __syncthreads();
                for (int p = 0; p < n; ++p) {
                    const int e = S.b_e[p];
                    float nl = S.b_onl[p];
                    if (S.pnode[e] >= 0) {
                        const int q = S.b_ppos[p];
                        if (q >= 0 && (q < p ? S.nt[S.b_e[q]] : S.b_ot[q]) != NEG_INF) {
                            const float prev = (merge && S.label[e] == S.label[S.b_e[q]]) ? S.b_ob[q] : S.b_ot[q];
                            nl = lse(nl, has_lm ? lw * S.delta[e] + prev : prev);
                        }
                        nl = nl + in[S.label[e]];
                    }
                    const float nb = S.b_ot[p] + in[blank];
                    __syncthreads();
                    if (lane == 0) {
                        S.nl[e] = nl;
                        S.nb[e] = nb;
                        S.nt[e] = lse(nb, nl);
                    }
                    __syncthreads();
                }
            }
        }
        float t0 = lane < n ? S.nt[S.b_e[lane]] : 0.f;
        float t1 = lane + 64 < n ? S.nt[S.b_e[lane + 64]] : 0.f;

        // ---- 3. child loop
        bool full = size == W;
        int bottom_slot = 0;
        float bottom_val = NEG_INF;
        auto find_bottom = [&]() {
            const uint64_t k0 = lane < size ? (((uint64_t)ord(t0) << 32) | (uint32_t)lane) : ~0ull;
            const uint64_t k1 = lane + 64 < size ? (((uint64_t)ord(t1) << 32) | (uint32_t)(lane + 64)) : ~0ull;
            const uint64_t m = wave_min_u64(k0 < k1 ? k0 : k1);
            bottom_slot = (int)(uint32_t)m;
            bottom_val = unord((uint32_t)(m >> 32));
        };
        auto slot_total = [&](int s) {
            return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s < 64 ? t0 : t1), s & 63));
        };
        if (full) find_bottom();
        const bool child_lane = lane < k && lane != blank;
        for (int i = 0; i < n; ++i) {
            if (S.b_reset[i]) continue;  // its oldp was reset by a rejected re-expansion: not a candidate
            const float ot = S.b_ot[i];
            if (!(ot > NEG_INF)) continue;
            if (full && !(ot > bottom_val)) break;  // sorted by ot and the bottom only rises: no later branch qualifies
            const int e = S.b_e[i];
            const float ob = S.b_ob[i];
            const int blab = S.label[e];
            float cv = NEG_INF;
            int cj = -1;
            if (child_lane) {
                const float prev = (merge && lane == blab) ? ob : ot;
                cv = in[lane] + (has_lm ? lw * (S.cache[e][lane] - S.score[e]) + prev : prev);
                cj = S.cbt[i * KMAX + lane];
            }
            uint64_t mask = __ballot(child_lane && (cj >= 0 || !full || cv > bottom_val));
            while (mask) {
                const int ind = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int j = __builtin_amdgcn_readlane(cj, ind);
                const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), ind));
                if (j >= 0) {
                    const int sl = S.b_slot[j];
                    if (sl >= 0 && slot_total(sl) != NEG_INF) continue;  // c->active()
                }
                if (v > NEG_INF && (size < W || v > bottom_val)) {
                    int s;
                    if (size == W) {
                        s = bottom_slot;  // it leaves the beam
                        const int src = S.slot_src[s];
                        if (src >= 0) S.b_slot[src] = -1;
                    } else {
                        s = size++;
                    }
                    if (lane == (s & 63)) {
                        if (s < 64) t0 = v;
                        else t1 = v;
                    }
                    S.slot_src[s] = -1 - (i * KMAX + ind);
                    full = size == W;
                    if (full) find_bottom();
                } else if (j >= 0) {
                    S.b_reset[j] = 1;  // c->oldp.reset() on a branch of this frame
                }
            }
        }

        // ---- 4. the new beam: storages, node ids, scorer state
        __syncthreads();
        for (int e = lane; e < W; e += 64) S.used[e] = 0;
        __syncthreads();
        for (int s = lane; s < size; s += 64) {
            const int src = S.slot_src[s];
            if (src >= 0) {
                S.used[S.b_e[src]] = 1;
                S.slot_e[s] = S.b_e[src];
            }
        }
        __syncthreads();
        {
            const bool f0_ = lane < W && !S.used[lane];
            const bool f1_ = lane + 64 < W && !S.used[lane + 64];
            const uint64_t m0 = __ballot(f0_), m1 = __ballot(f1_);
            if (f0_) S.freelist[lanes_below(m0)] = lane;
            if (f1_) S.freelist[__popcll(m0) + lanes_below(m1)] = lane + 64;
        }
        __syncthreads();
        // phase A: read everything a new entry needs (its parent's storage may be recycled below)
        const bool new0 = lane < size && S.slot_src[lane] < 0;
        const bool new1 = lane + 64 < size && S.slot_src[lane + 64] < 0;
        const uint64_t nm0 = __ballot(new0), nm1 = __ballot(new1);
        const int n_new = __popcll(nm0) + __popcll(nm1);
        int nn[2] = {0, 0}, npn[2] = {0, 0}, nlab_[2] = {0, 0}, ntr[2] = {0, 0}, nhl[2] = {0, 0};
        float ntot[2] = {t0, t1}, nlm[2] = {0.f, 0.f}, nsc[2] = {0.f, 0.f}, ndl[2] = {0.f, 0.f};
        uint32_t nh[2][HMAX];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool isnew = h == 0 ? new0 : new1;
            const int s = lane + 64 * h;
            int pnode = 0, ind = 0;
            if (isnew) {
                const int code = -1 - S.slot_src[s];
                const int pi = code / KMAX;
                ind = code - pi * KMAX;
                const int pe = S.b_e[pi];
                pnode = S.node[pe];
                nlab_[h] = ind;
                npn[h] = pnode;
#pragma unroll
                for (int j = 0; j < HMAX; ++j) nh[h][j] = S.hist[j][pe];
                nhl[h] = S.hlen[pe];
                if (has_lm) {
                    const float ps = S.score[pe];
                    const int ptr = S.trie[pe];
                    if (ind == lm.space_label) {
                        const uint32_t word = (uint32_t)trie_word(lm, ptr);
                        advance(lm, nh[h], &nhl[h], word);
                        nlm[h] = S.cache[pe][ind];
                        nsc[h] = nlm[h];
                        ntr[h] = 0;
                    } else {
                        nlm[h] = S.lm[pe];
                        nsc[h] = S.cache[pe][ind];
                        ntr[h] = ptr >= 0 && ptr < lm.n_trie_nodes ? lm.trie_child[(size_t)ptr * nlab + ind] : -1;
                    }
                    ndl[h] = nsc[h] - ps;
                }
            }
            // canonical node id of (parent node, label): the hash map, or a fresh node
            const uint32_t key = (uint32_t)(pnode * KMAX + ind + 1);
            uint64_t slot = fmix32(key) & hmask;
            int found = -1;
            if (isnew) {
                for (int64_t probe = 0; probe < hash_slots; ++probe) {
                    const unsigned long long v = hmap[slot];
                    if (v == 0ull) break;
                    if ((uint32_t)(v >> 32) == key) {
                        found = (int)(uint32_t)v;
                        break;
                    }
                    slot = (slot + 1) & hmask;
                }
            }
            const bool need = isnew && found < 0;
            const uint64_t nmask = __ballot(need);
            const int64_t id = n_nodes + lanes_below(nmask);
            n_nodes += __popcll(nmask);
            if (need) {
                if (id < node_cap) {
                    const unsigned long long val = ((unsigned long long)key << 32) | (uint32_t)id;
                    for (int64_t probe = 0; probe < hash_slots; ++probe) {
                        if (atomicCAS(&hmap[slot], 0ull, val) == 0ull) break;
                        slot = (slot + 1) & hmask;
                    }
                    arena[id] = (int32_t)(pnode * KMAX + ind);
                    found = (int)id;
                } else {
                    overflow = true;
                    found = 0;
                }
            }
            nn[h] = found;
        }
        __syncthreads();
        // phase B: write the new entries into free storages, in slot order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool isnew = h == 0 ? new0 : new1;
            if (!isnew) continue;
            const int s = lane + 64 * h;
            const int e = S.freelist[h == 0 ? lanes_below(nm0) : __popcll(nm0) + lanes_below(nm1)];
            S.slot_e[s] = e;
            S.node[e] = nn[h];
            S.pnode[e] = npn[h];
            S.label[e] = nlab_[h];
            S.nt[e] = ntot[h];
            S.nl[e] = ntot[h];
            S.nb[e] = NEG_INF;
            S.lm[e] = nlm[h];
            S.score[e] = nsc[h];
            S.delta[e] = ndl[h];
            S.trie[e] = ntr[h];
            S.hlen[e] = nhl[h];
#pragma unroll
            for (int j = 0; j < HMAX; ++j) S.hist[j][e] = nh[h][j];
        }
        // old survivors' new totals are already in their storages (first loop)
        __syncthreads();
        if (has_lm && n_new > 0) fill_cache(n_new);
    }

    // ---- end of utterance: expand_state_end, best leaf (first maximum in slot order), LabelSeq(merge_repeated)
    uint64_t best = ~0ull;
    for (int s = lane; s < size; s += 64) {
        const int e = S.slot_e[s];
        float total = S.nt[e];
        if (has_lm) {
            uint32_t h[HMAX];
#pragma unroll
            for (int j = 0; j < HMAX; ++j) h[j] = S.hist[j][e];
            int hl = S.hlen[e];
            float d = 0.f;
            if (S.trie[e] != 0) {  // a pending word (node 0 = the empty word)
                const uint32_t word = (uint32_t)trie_word(lm, S.trie[e]);
                d += ngram_score(lm, h, hl, word);
                advance(lm, h, &hl, word);
            }
            d += ngram_score(lm, h, hl, (uint32_t)lm.eos);
            const float previous = S.score[e];
            const float lms = S.lm[e] + d;
            total += lw * (lms - previous);
        }
        S.slot_tot[s] = total;
        const uint64_t key = ((uint64_t)~ord(total) << 32) | (uint32_t)s;
        best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    __syncthreads();
    const int top = (int)(uint32_t)best;
    const int top_node = S.node[S.slot_e[top]];
    if (lane == 0) {
        int count = 0, prev = -1, c = top_node;
        for (int step = 0; c > 0 && step <= len; ++step) {
            const int pp = arena[c];
            const int lab = pp & (KMAX - 1);
            if (!merge || lab != prev) ++count;
            prev = lab;
            c = pp >> 6;
        }
        S.scalar[0] = count;
    }
    __syncthreads();
    const int count = S.scalar[0];
    int32_t* row = out + (size_t)b * t_max;
    for (int i = count + lane; i < t_max; i += 64) row[i] = -1;
    if (lane == 0) {
        int pos = count - 1, prev = -1, c = top_node;
        for (int step = 0; c > 0 && step <= len; ++step) {
            const int pp = arena[c];
            const int lab = pp & (KMAX - 1);
            if (!merge || lab != prev) {
                if (pos >= 0 && pos < t_max) row[pos] = lab;
                --pos;
            }
            prev = lab;
            c = pp >> 6;
        }
        out_len[b] = overflow ? -1 : min(count, t_max);
        if (log_prob) log_prob[b] = S.slot_tot[top];
    }
}

}  // namespace

extern "C" size_t sl_ctc_beam_search_workspace_bytes(int batch, int t_max, int k, int beam_width) {
    return beam_workspace_bytes(batch, t_max, k, beam_width);
}

extern "C" int sl_ctc_beam_search(const float* probs, const int32_t* lengths, int batch, int t_max, int k, int blank,
                                  int beam_width, int merge_repeated, float eps, const sl_beam_lm* lm, int32_t* out,
                                  int32_t* out_len, float* log_prob, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    static const BeamWords words = {"sl_ctc_beam_search", "t_max", "class", "alphabet"};
    SL_CHECK_ARG(probs && lengths && out && out_len && workspace, "sl_ctc_beam_search: null pointer");
    SL_CHECK_ARG(blank >= 0 && blank < k, "sl_ctc_beam_search: blank %d outside [0, %d)", blank, k);
    const int rc = beam_check_args(words, batch, t_max, k, beam_width, lm, k - 1);
    if (rc != SL_OK) return rc;
    if (lm && blank != k - 1) {
        sl_set_error("sl_ctc_beam_search: with a language model the blank must be the last class (k - 1)");
        return SL_ERR_UNSUPPORTED;
    }
    const hipStream_t s = (hipStream_t)stream;
    const int ws_rc = beam_clear_workspace(words.fn, workspace, workspace_bytes,
                                           beam_workspace_bytes(batch, t_max, k, beam_width), s);
    if (ws_rc != SL_OK) return ws_rc;
    const BeamSizes z = beam_sizes_of(t_max, beam_width);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(batch), dim3(64), 0, s, probs, lengths, t_max, k, blank, beam_width,
                       merge_repeated ? 1 : 0, eps, lm ? 1 : 0, lm ? *lm : beam_lm_none(), out, out_len, log_prob,
                       (uint8_t*)workspace, z.node_cap, z.hash_slots, z.stride);
    return sl_check_launch(words.fn);
}
