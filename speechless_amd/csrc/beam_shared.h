// beam_shared.h -- what the two beam searches (ctc_beam.hip, asg_beam.hip) share, each piece ONCE.  Both kernels use the first
// two device items below as far as the n-gram look-up, advance and trie_word, the workspace layout and the host side.  The
// scorer state St with its three functions, BeamStorages, NodeTable and the backtrace are asg_beam.hip's so far:
// ctc_beam.hip still writes them out by hand, in the same operation order (it ran 1 % slower on them: DESIGN.md 3.3).
//   - the limits and the staging chunk (WMAX, KMAX, CH), NEG_INF, lanes_below, the monotone float <-> uint32 map both
//     searches order their candidates by;
//   - the device side of the scorer: the open-addressed n-gram table of sl_host_scorer_export (include/speechless_host.h),
//     NGramModel::score with back-off, the history shift, the word of a trie node, and the scorer state of a prefix (St) with
//     the three things done to it: expand, step_into_child, expand_end_delta.  The operation order that
//     include/speechless_hip.h defines bit for bit is the one of expand(), stated there;
//   - the per-storage LDS arrays of a beam (BeamStorages), their root and their free list;
//   - the per-utterance workspace: the node arena, the (parent node, label) -> node hash map (NodeTable) and the backtrace;
//   - on the host: the argument and language-model checks, the workspace size and its clearing, the "no model" sl_beam_lm.
// Every translation unit that includes it compiles with contraction off: the host scorer rounds each operation on its own.
// No helper here holds a barrier: those stay in the kernels.  How a fresh node id is allocated stays there too, next to the
// kernel's argument for its uniformity.
#pragma once
#include "common.h"

#pragma clang fp contract(off)  // lm_weight * delta + previous is two roundings on the host

namespace {

constexpr int WMAX = 128;  // beam width limit
constexpr int KMAX = 64;   // classes: one lane each
constexpr int CH = 16;     // frames per LDS staging chunk
constexpr int HMAX = 5;    // words of language-model history (order <= 6)
constexpr float NEG_INF = -__builtin_huge_valf();

__device__ __forceinline__ int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// monotone float -> uint32 (-0 == +0, as the host's comparisons see them)
__device__ __forceinline__ uint32_t ord(float f) {
    const uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------------------------------------------- the scorer
// speechless_host.h, sl_host_scorer_export: home slot of a key
__device__ __forceinline__ uint32_t ngram_hash(const uint32_t (&w)[6]) {
    uint32_t h = 0x811C9DC5u;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        h = (h ^ w[i]) * 0x01000193u;
        h ^= h >> 15;
    }
    return fmix32(h);
}

__device__ bool ngram_find(const sl_beam_lm& lm, const uint32_t (&w)[6], float* prob, float* backoff) {
    const uint64_t mask = (uint64_t)lm.ngram_slots - 1;
    uint64_t i = ngram_hash(w) & mask;
    for (int64_t probe = 0; probe < lm.ngram_slots; ++probe) {
        const u32x4* e = (const u32x4*)(lm.ngrams + i * 8);
        const u32x4 a = e[0], b = e[1];
        if (a.x == 0u) return false;
        if (a.x == w[0] && a.y == w[1] && a.z == w[2] && a.w == w[3] && b.x == w[4] && b.y == w[5]) {
            *prob = __uint_as_float(b.z);
            *backoff = __uint_as_float(b.w);
            return true;
        }
        i = (i + 1) & mask;
    }
    return false;
}

// NGramModel::score: log10 P(word | history) with back-off.  r: history right-aligned (r[4] = the latest word), hlen of it.
__device__ float ngram_score(const sl_beam_lm& lm, const uint32_t (&r)[HMAX], int hlen, uint32_t word) {
    int clen = min(hlen, lm.order - 1);
    float backoff = 0.f;
    for (;;) {
        uint32_t w[6];
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = j >= 5 - clen ? r[j] : 0u;
        w[5] = word;
        w[0] |= (uint32_t)(clen + 1) << 29;
        float p, bo;
        if (ngram_find(lm, w, &p, &bo)) return backoff + p;
        if (clen == 0) return backoff + lm.oov_score;
        w[0] = (uint32_t)clen << 29;
#pragma unroll
        for (int j = 1; j < 6; ++j) w[j] = j >= 6 - clen ? r[j - 1] : 0u;
        if (ngram_find(lm, w, &p, &bo)) backoff += bo;
        --clen;
    }
}

__device__ __forceinline__ void advance(const sl_beam_lm& lm, uint32_t (&r)[HMAX], int* hlen, uint32_t word) {
#pragma unroll
    for (int j = 0; j < HMAX - 1; ++j) r[j] = r[j + 1];
    r[HMAX - 1] = word;
    *hlen = min(*hlen + 1, lm.order - 1);
}

__device__ __forceinline__ int trie_word(const sl_beam_lm& lm, int node) {
    return node >= 0 && node < lm.n_trie_nodes ? lm.trie_word[node] : 0;
}

struct St {  // scorer state of a prefix: lm = the score behind its last whole word, score = lm + the best word its pending
    float lm, score;  // letters can still become, trie = the node of those letters, h / hlen = the words before them
    int trie, hlen;
    uint32_t h[HMAX];
};

// The scorer's expand_state for one character c of an alphabet of nlab; returns the delta (the new score - the old one).
// THE operation order of both searches, every operation rounded on its own:
//   at a space: v = lm; if (the pending letters are a word) v += valid_word_count_weight; v += word_count_weight;
//               score = v + log10 P(word | history);   the word enters the history, lm = score, the trie restarts;
//   otherwise:  score = trie_min[trie][c] + lm (oov_score off the trie); the trie steps to its child.
__device__ __forceinline__ float expand(const sl_beam_lm& lm, int nlab, St& s, int c) {
    float ns;
    if (c == lm.space_label) {
        const uint32_t word = (uint32_t)trie_word(lm, s.trie);
        const float d = ngram_score(lm, s.h, s.hlen, word);
        float v = s.lm;
        if (word != 0u) v += lm.valid_word_count_weight;
        v += lm.word_count_weight;
        ns = v + d;
        s.lm = ns;
        s.trie = 0;
        advance(lm, s.h, &s.hlen, word);
    } else {
        const bool in = s.trie >= 0 && s.trie < lm.n_trie_nodes;
        const float mu = in ? lm.trie_min[(size_t)s.trie * nlab + c] : lm.oov_score;
        ns = mu + s.lm;
        s.trie = in ? lm.trie_child[(size_t)s.trie * nlab + c] : -1;
    }
    const float delta = ns - s.score;
    s.score = ns;
    return delta;
}

// expand() for a caller that already holds the score behind c (a beam entry caches expand()'s score for each of its
// children): what is left is the trie step or, at a space, the history shift.  No n-gram query, no arithmetic.
__device__ __forceinline__ void step_into_child(const sl_beam_lm& lm, int nlab, St& s, int c, float score_behind_c) {
    if (c == lm.space_label) {
        advance(lm, s.h, &s.hlen, (uint32_t)trie_word(lm, s.trie));
        s.trie = 0;
        s.lm = score_behind_c;
    } else {
        const bool in = s.trie >= 0 && s.trie < lm.n_trie_nodes;
        s.trie = in ? lm.trie_child[(size_t)s.trie * nlab + c] : -1;
    }
    s.score = score_behind_c;
}

// The scorer's expand_state_end: the pending word (trie node 0 = the empty word), then </s>.  Returns the delta.
__device__ __forceinline__ float expand_end_delta(const sl_beam_lm& lm, St s) {
    float d = 0.f;
    if (s.trie != 0) {
        const uint32_t word = (uint32_t)trie_word(lm, s.trie);
        d += ngram_score(lm, s.h, s.hlen, word);
        advance(lm, s.h, &s.hlen, word);
    }
    d += ngram_score(lm, s.h, s.hlen, (uint32_t)lm.eos);
    return (s.lm + d) - s.score;
}

// ------------------------------------------------------------------------------------------- the storages of a beam
// One storage per beam entry, in LDS (the base of a kernel's Lds): the prefix's node, its parent's node and its last label,
// its scorer state and, with a language model, the scorer's score behind each of its children.
struct BeamStorages {
    int node[WMAX], pnode[WMAX], label[WMAX], trie[WMAX], hlen[WMAX];
    float lm[WMAX], score[WMAX];
    uint32_t hist[HMAX][WMAX];
    float cache[WMAX][KMAX];
    int used[WMAX], freelist[WMAX];
};

__device__ __forceinline__ St load_state(const BeamStorages& B, int e) {
    St s;
    s.lm = B.lm[e];
    s.score = B.score[e];
    s.trie = B.trie[e];
    s.hlen = B.hlen[e];
#pragma unroll
    for (int j = 0; j < HMAX; ++j) s.h[j] = B.hist[j][e];
    return s;
}

__device__ __forceinline__ void store_state(BeamStorages& B, int e, const St& s) {
    B.lm[e] = s.lm;
    B.score[e] = s.score;
    B.trie[e] = s.trie;
    B.hlen[e] = s.hlen;
#pragma unroll
    for (int j = 0; j < HMAX; ++j) B.hist[j][e] = s.h[j];
}

// storage 0 = node 0 = the empty prefix, behind <s>; its "last label" is the search's own.  One thread.
__device__ __forceinline__ void init_root(BeamStorages& B, int32_t* arena, int root_label, int bos) {
    arena[0] = -1;
    B.node[0] = 0;
    B.pnode[0] = -1;
    B.label[0] = root_label;
    B.lm[0] = B.score[0] = 0.f;
    B.trie[0] = 0;
    B.hlen[0] = 1;
    for (int j = 0; j < HMAX; ++j) B.hist[j][0] = j == HMAX - 1 ? (uint32_t)bos : 0u;
    B.freelist[0] = 0;
}

// freelist[0 ..) = the storages e < W with used[e] == 0, ascending.  One whole wave (WMAX = two lanes' worth).
__device__ __forceinline__ void build_freelist(const int* used, int W, int* freelist, int lane) {
    const bool f0 = lane < W && !used[lane];
    const bool f1 = lane + 64 < W && !used[lane + 64];
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
    if (f0) freelist[lanes_below(m0)] = lane;
    if (f1) freelist[__popcll(m0) + lanes_below(m1)] = lane + 64;
}

// -------------------------------------------------------------------------------------------- the node table
// per-utterance workspace of a search: the node arena the backtrace walks, then the (parent node, label) -> node hash map
struct BeamSizes {
    int64_t node_cap, hash_slots, stride;
};

inline BeamSizes beam_sizes_of(int t_max, int beam_width) {
    BeamSizes z;
    z.node_cap = (int64_t)t_max * beam_width + 1;  // at most beam_width new nodes per frame
    z.hash_slots = 16;
    while (z.hash_slots < 2 * z.node_cap) z.hash_slots *= 2;
    z.stride = ((z.node_cap * 4 + 7) & ~(int64_t)7) + z.hash_slots * 8;
    return z;
}

// A node is a prefix: arena[id] names its parent node and its last label; the map gives a (parent, label) its one id for the
// whole utterance, so that a prefix that left the beam and comes back is the same node.  The three encodings:
__device__ __forceinline__ int32_t arena_word(int parent, int label) { return (int32_t)(parent * KMAX + label); }
__device__ __forceinline__ uint32_t node_key(int parent, int label) { return (uint32_t)(parent * KMAX + label + 1); }  // never 0
__device__ __forceinline__ int word_label(int32_t w) { return w & (KMAX - 1); }
__device__ __forceinline__ int word_parent(int32_t w) { return w >> 6; }  // the root's word is -1: parent -1 ends a walk
static_assert(KMAX == 1 << 6, "word_parent shifts by log2(KMAX)");

struct NodeTable {
    int32_t* arena;
    unsigned long long* hmap;  // 0: empty, else key << 32 | id
    uint64_t hmask;
    int64_t node_cap, hash_slots;

    __device__ __forceinline__ NodeTable(uint8_t* ws, int b, const BeamSizes& z)
        : arena((int32_t*)(ws + (size_t)b * z.stride)),
          hmap((unsigned long long*)(ws + (size_t)b * z.stride + (((size_t)z.node_cap * 4 + 7) & ~(size_t)7))),
          hmask((uint64_t)z.hash_slots - 1), node_cap(z.node_cap), hash_slots(z.hash_slots) {}

    // The id under `key`, or -1 with `slot` at the first empty slot of the key's chain.
    // The map is written with atomics, which complete at L2, while a plain vector load may be served by a line that L1
    // fetched before the insert -- and would then hand a returning prefix a second id.  So the probe is an agent-scope
    // atomic load (relaxed: a slot is one 64-bit word, nothing else is published through it), which L2 serves.
    __device__ __forceinline__ int find(uint32_t key, uint64_t& slot) const {
        slot = fmix32(key) & hmask;
        for (int64_t probe = 0; probe < hash_slots; ++probe) {
            const unsigned long long v = __hip_atomic_load(&hmap[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == 0ull) break;
            if ((uint32_t)(v >> 32) == key) return (int)(uint32_t)v;
            slot = (slot + 1) & hmask;
        }
        return -1;
    }

    // The fresh node `id` (< node_cap: the caller's check) = (parent, label), from the slot find() left: several threads of a
    // frame insert different keys at once, so a slot may have been taken since.
    __device__ __forceinline__ void insert(uint64_t slot, uint32_t key, int id, int parent, int label) const {
        const unsigned long long val = ((unsigned long long)key << 32) | (uint32_t)id;
        for (int64_t probe = 0; probe < hash_slots; ++probe) {
            if (atomicCAS(&hmap[slot], 0ull, val) == 0ull) break;
            slot = (slot + 1) & hmask;
        }
        arena[id] = arena_word(parent, label);
    }
};

// The backtrace from `node` to the root, by ONE thread; at most len labels (a node per frame).  merge: a label that repeats
// its predecessor is not counted or written (CTC's merge_repeated).  write_labels fills row[0 .. count) as far as t_max goes.
__device__ __forceinline__ int count_labels(const int32_t* arena, int node, int len, bool merge) {
    int count = 0, prev = -1;
    for (int step = 0; node > 0 && step <= len; ++step) {
        const int32_t w = arena[node];
        if (!merge || word_label(w) != prev) ++count;
        prev = word_label(w);
        node = word_parent(w);
    }
    return count;
}

__device__ __forceinline__ void write_labels(const int32_t* arena, int node, int len, bool merge, int32_t* row, int count,
                                             int t_max) {
    int pos = count - 1, prev = -1;
    for (int step = 0; node > 0 && step <= len; ++step) {
        const int32_t w = arena[node];
        if (!merge || word_label(w) != prev) {
            if (pos >= 0 && pos < t_max) row[pos] = word_label(w);
            --pos;
        }
        prev = word_label(w);
        node = word_parent(w);
    }
}

// ------------------------------------------------------------------------------------------------------ host side
// The words of an entry point's error texts.  (More than the function's name only so that every text stays what it was: the
// two entry points say t_max / t_out, class / grapheme and alphabet / characters.)
struct BeamWords {
    const char *fn, *t, *lane, *scored;  // its name, its frame-count argument, what a lane holds, what the model scores
};

inline size_t beam_workspace_bytes(int batch, int t, int k, int beam_width) {
    if (batch <= 0 || t <= 0 || k < 2 || k > KMAX || beam_width < 1 || beam_width > WMAX) return 0;
    if ((int64_t)t * beam_width + 1 >= ((int64_t)1 << 25)) return 0;
    return (size_t)batch * beam_sizes_of(t, beam_width).stride;
}

inline sl_beam_lm beam_lm_none() {
    sl_beam_lm none = {};
    none.order = 1;
    none.space_label = -1;
    return none;
}

// The checks both searches make of their shape and of the model (lm may be null); n_scored_labels: the model's alphabet.
inline int beam_check_args(const BeamWords& w, int batch, int t, int k, int beam_width, const sl_beam_lm* lm,
                           int n_scored_labels) {
    SL_CHECK_ARG(batch > 0 && t > 0, "%s: need batch, %s > 0", w.fn, w.t);
    if (k < 2 || k > KMAX) {
        sl_set_error("%s: k = %d outside 2 <= k <= %d (one lane per %s)", w.fn, k, KMAX, w.lane);
        return SL_ERR_UNSUPPORTED;
    }
    if (beam_width < 1 || beam_width > WMAX) {
        sl_set_error("%s: beam width %d outside [1, %d]", w.fn, beam_width, WMAX);
        return SL_ERR_UNSUPPORTED;
    }
    if ((int64_t)t * beam_width + 1 >= ((int64_t)1 << 25)) {
        sl_set_error("%s: %s * beam_width = %lld too large (node ids are 25-bit)", w.fn, w.t, (long long)t * beam_width);
        return SL_ERR_UNSUPPORTED;
    }
    if (lm) {
        SL_CHECK_ARG(lm->trie_child && lm->trie_min && lm->trie_word && lm->ngrams && lm->n_trie_nodes > 0,
                     "%s: incomplete language model tables", w.fn);
        SL_CHECK_ARG(lm->ngram_slots >= 1 && (lm->ngram_slots & (lm->ngram_slots - 1)) == 0,
                     "%s: ngram_slots must be a power of two", w.fn);
        SL_CHECK_ARG(lm->space_label >= -1 && lm->space_label < n_scored_labels, "%s: space label outside the %s", w.fn,
                     w.scored);
        if (lm->order < 1 || lm->order > HMAX + 1) {
            sl_set_error("%s: language model order %d outside [1, %d]", w.fn, lm->order, HMAX + 1);
            return SL_ERR_UNSUPPORTED;
        }
    }
    return SL_OK;
}

// The workspace of a call: large enough, and cleared (the hash maps start empty).
inline int beam_clear_workspace(const char* fn, void* workspace, size_t workspace_bytes, size_t need, hipStream_t s) {
    if (workspace_bytes < need) {
        sl_set_error("%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
        return SL_ERR_WORKSPACE_TOO_SMALL;
    }
    if (hipMemsetAsync(workspace, 0, need, s) != hipSuccess) {
        sl_set_error("%s: workspace clear failed", fn);
        return SL_ERR_LAUNCH_FAILED;
    }
    return SL_OK;
}

}  // namespace
