// Label-sequence trie of the device beam searches (ctc_beam.hip, rnnt_beam.hip): one node per label sequence of an utterance
// (node 0 = the empty sequence; after a compaction, beam_select.h, the root of what is left, which keeps its label), found by an
// open-addressing (parent node, label) -> node table, and the sequence order of the searches' exact-tie rule (lexicographic, a proper
// prefix first).  Written and read by one workgroup: plain (non-restrict)
// pointers, ordered by __syncthreads.
#pragma once
#include "common.h"

namespace beam_trie {

constexpr unsigned long long EMPTY = ~0ull;  // free slot of the (parent, label) table

struct Trie { int* parent; int* label; int* depth; };

// A label sequence given as (node, extra): the node's sequence, followed by `extra` when extra >= 0.
struct Seq { int n, x; };
__device__ __forceinline__ int seq_len(const Trie& tr, Seq s) { return tr.depth[s.n] + (s.x >= 0); }
__device__ __forceinline__ int seq_last(const Trie& tr, Seq s) { return s.x >= 0 ? s.x : tr.label[s.n]; }
__device__ __forceinline__ Seq seq_up(const Trie& tr, Seq s) { return s.x >= 0 ? Seq{s.n, -1} : Seq{tr.parent[s.n], -1}; }
__device__ __forceinline__ bool seq_eq(const Trie& tr, Seq a, Seq b) {
  if ((a.x >= 0) == (b.x >= 0)) return a.n == b.n && a.x == b.x;
  if (a.x >= 0) { Seq t = a; a = b; b = t; }  // a real node, b = (node, extra)
  return tr.parent[a.n] == b.n && tr.label[a.n] == b.x;
}
// lexicographic a < b (a proper prefix is smaller), as std::vector's operator<
__device__ inline bool seq_less(const Trie& tr, Seq a, Seq b) {
  int la = seq_len(tr, a), lb = seq_len(tr, b);
  const bool b_longer = lb > la;
  for (; la > lb; --la) a = seq_up(tr, a);
  for (; lb > la; --lb) b = seq_up(tr, b);
  if (seq_eq(tr, a, b)) return b_longer;  // one is a prefix of the other (or they are equal)
  int ea = 0, eb = 0;
  while (!seq_eq(tr, a, b)) { ea = seq_last(tr, a); eb = seq_last(tr, b); a = seq_up(tr, a); b = seq_up(tr, b); }
  return ea < eb;
}

__host__ __device__ __forceinline__ unsigned hash(int par, int c, unsigned mask) {
  return ((unsigned)par * 0x9E3779B1u ^ ((unsigned)c + 0x7F4A7C15u) * 0x85EBCA77u) & mask;
}
__host__ __device__ __forceinline__ unsigned long long key(int par, int c) { return ((unsigned long long)(unsigned)par << 32) | (unsigned)c; }

// node of (par, c) or -1 (also called by host code: the n-gram tables of ngram_lm.h have this layout)
__host__ __device__ inline int lookup(const unsigned long long* hk, const int* hv, unsigned hcap, int par, int c) {
  const unsigned long long k = key(par, c);
  unsigned h = hash(par, c, hcap - 1);
  for (unsigned probe = 0; probe < hcap; ++probe, h = (h + 1) & (hcap - 1)) {
    const unsigned long long kk = hk[h];
    if (kk == k) return hv[h];
    if (kk == EMPTY) return -1;
  }
  return -1;
}
__device__ inline void insert(unsigned long long* hk, int* hv, unsigned hcap, int par, int c, int node) {
  const unsigned long long k = key(par, c);
  unsigned h = hash(par, c, hcap - 1);
  for (unsigned probe = 0; probe < hcap; ++probe, h = (h + 1) & (hcap - 1))
    if (atomicCAS(&hk[h], EMPTY, k) == EMPTY) { hv[h] = node; return; }
}

// ---- the stable prefix of a carried beam (the chunked searches' commit), run by ONE wave: lane i holds the node of live row i ----
// The deepest node that is an ancestor-or-self of every live lane's node.  Lane 0 must be live.  Every lane walks up to the smallest
// depth, then all walk up together until a ballot says they agree: O(depth below the answer) parent reads per lane.
__device__ inline int common_ancestor(const Trie& tr, int node, bool live) {
  int dmin = live ? tr.depth[node] : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dmin = min(dmin, __shfl_xor(dmin, o, 64));
  if (live)
    for (int d = tr.depth[node]; d > dmin; --d) node = tr.parent[node];
  for (;;) {
    const int first = __shfl(node, 0, 64);
    if (__ballot(live && node != first) == 0ull) return first;
    if (live) node = tr.parent[node];  // (all at one depth > 0 here: the root is common to all)
  }
}
// Labels of `target`'s sequence from depth *committed on -> out[0 .. n), n = min(depth(target) - *committed, width) >= 0, the rest of
// out[0 .. width) = pad; *count = n, *committed += n (labels that did not fit come with the next commit).  `target` is wave uniform.
__device__ inline void commit_labels(const Trie& tr, int target, int lane, int32_t* committed, int32_t* out, int32_t* count, int width,
                                     int pad) {
  const int have = max(*committed, 0);
  const int n = max(min(tr.depth[target] - have, width), 0), upto = have + n;
  for (int pos = n + lane; pos < width; pos += 64) out[pos] = pad;
  if (lane == 0) {
    int t = target;
    for (int d = tr.depth[t]; d > upto; --d) t = tr.parent[t];
    for (int d = upto; d > have; --d, t = tr.parent[t]) out[d - have - 1] = tr.label[t];
    *count = n;
    *committed = upto;
  }
}

// table slots for an utterance of at most `nmax` nodes (load factor <= 1/2)
inline unsigned table_cap(long nmax) {
  unsigned long long cap = 64;
  while (cap < 2ull * (unsigned long long)nmax) cap <<= 1;
  return (unsigned)cap;
}

}  // namespace beam_trie
