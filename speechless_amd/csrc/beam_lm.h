// beam_lm.h -- the device side of the beam-search scorer that ctc_beam.hip and asg_beam.hip share: the open-addressed
// n-gram table of sl_host_scorer_export (include/speechless_host.h), NGramModel::score with back-off, the history shift,
// the word of a trie node, the monotone float <-> uint32 map both searches order their candidates by, and the workspace layout.
// Every translation unit that includes it compiles with contraction off: the host scorer rounds each operation on its own.
#pragma once
#include "common.h"

#pragma clang fp contract(off)  // lm_weight * delta + previous is two roundings on the host

namespace {

constexpr int HMAX = 5;  // words of language-model history (order <= 6)

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

}  // namespace
