// pgq_pack.h — the bit-packed copy of the padded adjacency: a 16-byte group holds K ids of ONE list, each
// W = 128 / K bits wide, little-endian across the group's four words (id k at bits k W .. k W + W - 1; the bits past
// K W are zero).  K = 4 is the 32-bit padded layout itself.  Shared by the upload kernel that writes the layout, the walk
// that reads it (pgq_walk.h) and the CPU test of the layout, so it compiles without HIP too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PGQ_HD __host__ __device__ __forceinline__
#else
#define PGQ_HD inline
#endif

namespace pgq {

// ids per 16-byte group for a graph of V vertices (ids < V): 6 x 21 bits up to 2^21 vertices, 5 x 25 bits up to 2^25
// when `with5` (option meet_pack = 2), else 4 (no packed copy: the 32-bit layout)
PGQ_HD int pack_k_for(int64_t V, bool with5) {
	return V <= (int64_t(1) << 21) ? 6 : (with5 && V <= (int64_t(1) << 25) ? 5 : 4);
}

// groups of a packed list of `len` entries whose lists are aligned to `align` groups (align >= 1): ceil(len / (K align))
// x align; an empty list has none
PGQ_HD uint32_t pack_list_groups(uint32_t len, int K, uint32_t align) {
	const uint32_t per = (uint32_t)K * align;
	return (len + per - 1u) / per * align;
}

// id k of a packed group w[0..3]: one funnel shift (v_alignbit) and a mask when it straddles two words
template <int K> PGQ_HD uint32_t pack_get(const uint32_t w[4], int k) {
	constexpr int W = 128 / K;
	const int b = k * W, i = b >> 5, o = b & 31;
	if constexpr (W == 32) {
		return w[i];
	} else {
		const uint64_t both = (uint64_t)w[i] | (i + 1 < 4 ? (uint64_t)w[i + 1] << 32 : 0ull);
		return (uint32_t)(both >> o) & ((1u << W) - 1u);
	}
}

// packs ids[0..K) (each < 2^W) into w[0..3]
template <int K> PGQ_HD void pack_put(const uint32_t *ids, uint32_t w[4]) {
	constexpr int W = 128 / K;
	w[0] = w[1] = w[2] = w[3] = 0u;
	for (int k = 0; k < K; k++) {
		const int b = k * W, i = b >> 5, o = b & 31;
		w[i] |= ids[k] << o;
		if (o + W > 32) w[i + 1] |= ids[k] >> (32 - o);
	}
}

// group g (counted from the list's first group) of the packed list adj[0 .. len): entries g K .. g K + K - 1, the
// positions past the list's end repeating its last entry (len > 0)
template <int K> PGQ_HD void pack_list_group(const int32_t *adj, int64_t len, uint32_t g, uint32_t w[4]) {
	uint32_t ids[K];
	const int64_t i0 = (int64_t)g * K;
	for (int k = 0; k < K; k++) ids[k] = (uint32_t)adj[i0 + k < len ? i0 + k : len - 1];
	pack_put<K>(ids, w);
}

// ---- the order inside a packed list, and the two parts it is walked in -----------------------------------
// A two-hop walk ends at its first entry that lies in the other endpoint's one-hop list, and an entry is the likelier to
// be such a member the longer its own list in the OTHER direction is.  The packed copies are private to the hop-count
// walks, so the upload orders every packed list by non-increasing pack_order_bucket of that length (stable: equal buckets
// keep the CSR's order), and a row walks the first quarter of the groups of ALL its lists (the heads) before the rest.

// floor(log2(max(len, 1))): 0 .. 31
PGQ_HD int pack_order_bucket(uint32_t len) { return 31 - __builtin_clz(len | 1u); }

// groups in the head of a list of `ng` groups (ng = ceil(len / K): the groups the walk reads, not the aligned count); the
// tail is the other ng - pack_head_groups(ng)
PGQ_HD uint32_t pack_head_groups(uint32_t ng) { return (ng + 3u) >> 2; }

// Part `part` (0: head, 1: tail) of a list of `len` entries: its first group counted from the list's first, its groups and
// the list entries it holds (the padding of the last group belongs to nobody).  split = false: part 0 is the whole list.
struct PackPart {
	uint32_t first, groups, entries;
};
PGQ_HD PackPart pack_part(uint32_t len, int K, int part, bool split) {
	const uint32_t ng = (len + (uint32_t)(K - 1)) / (uint32_t)K;
	const uint32_t h = split ? pack_head_groups(ng) : ng;
	const uint32_t he = h * (uint32_t)K < len ? h * (uint32_t)K : len; // entries of the head
	return part == 0 ? PackPart { 0u, h, he } : PackPart { h, ng - h, len - he };
}

} // namespace pgq
