// The maximum-clique baseline PMC(...) of the reference's evaluation (GMF_PointDSC/baseline_scripts/baseline_3DMatch.py:56-77),
// batched over ragged pairs and exact: the pairwise-compatibility graph, a maximum clique of it, Kabsch on its members.
//
//   k_pmc_graph     rows on threads, the columns streamed through LDS; a thread packs 64 comparisons into one word of its bit row
//                   and counts its degree.  fp32, every operation rounded on its own (built with -ffp-contract=off)
//   k_pmc_order     one workgroup per pair peels the graph by core level: order[p] = the row removed p-th, ties by row.  A vertex
//                   has at most `degeneracy` neighbours behind it in that order, and core numbers do not decrease along it
//   k_pmc_renumber  the bit matrix in that order: bit q of row p = edge (order[p], order[q])
//   k_pmc_greedy    one wave per start vertex: take the last candidate (the highest core number) until none is left; the largest
//                   goes in by a 64-bit atomicMax on (size, ~start), which does not depend on arrival order
//   k_pmc_search    one wave per root, roots by ticket: branch and bound over the root's later neighbours, greedy colour bound
//   k_pmc_finish    labels from the winner's members, size / exact / steps
// and k_sm_pose of spectral_kernels.hip for the pose.
//
// A vertex set over the pair's <= 8192 vertices is two 64-bit words per lane (words lane and lane + 64); an intersection is a
// lane-wise AND with a row of the bit matrix.  The search keeps no stack of such sets: the clique so far is a list in LDS, and
// the candidates left at a level are recomputed from it on the way back (branching is in vertex order, so they are the common
// neighbours behind the vertex tried last).  A root with few candidates renumbers them and does keep its sets, in LDS
// (k_pmc_search).
//
// Which clique.  Every key is (size << 32) | ~vertex.  A root's search starts with own = the starting clique's size and records only
// strictly larger cliques; it cuts a branch only when its bound is below the incumbent's size or not above own.  Neither cut can
// remove a clique of size omega that is larger than own, so a root that has one finds the first in its search order, whatever
// the other waves do; the largest key is then the smallest such root.  If none is larger than the starting clique, that one
// stays.  So the answer is a function of the pair's graph alone whenever the budget did not end the search.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kabsch.hpp"
#include "launchers_clique.hpp"
#include "launchers_spectral.hpp"

namespace gmf {

namespace {

typedef unsigned long long u64;

// the rows of pair `pair`; false: empty, or beyond the caller's bounds (not computed)
GMF_DEVINL bool pmc_pair(const int* __restrict__ offsets, int pair, long long total_rows, int max_n, int& r0, int& n) {
  r0 = offsets[pair];
  n = offsets[pair + 1] - r0;
  return n > 0 && n <= max_n && r0 >= 0 && (long long)offsets[pair + 1] <= total_rows;
}

struct WSet { u64 lo, hi; };      // words `lane` and `lane + 64` of a vertex set

GMF_DEVINL WSet pmc_row(const u64* __restrict__ row, int W, int lane) {
  WSet s;
  s.lo = lane < W ? row[lane] : 0ull;
  s.hi = lane + 64 < W ? row[lane + 64] : 0ull;
  return s;
}
GMF_DEVINL u64 pmc_above(int word, int v) {      // the bits of word `word` that stand for vertices > v
  const int w = v >> 6, b = v & 63;
  return word > w ? ~0ull : (word == w ? (b == 63 ? 0ull : (~0ull << (b + 1))) : 0ull);
}
GMF_DEVINL void pmc_and(WSet& a, const WSet& b) { a.lo &= b.lo; a.hi &= b.hi; }
GMF_DEVINL void pmc_drop(WSet& a, int v, int lane) {
  const u64 bit = 1ull << (v & 63);
  if ((v >> 6) == lane) a.lo &= ~bit;
  if ((v >> 6) == lane + 64) a.hi &= ~bit;
}
GMF_DEVINL bool pmc_empty(const WSet& s) { return __ballot((s.lo | s.hi) != 0ull) == 0ull; }
GMF_DEVINL int pmc_count(const WSet& s) {
  int c = __popcll(s.lo) + __popcll(s.hi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}
// the smallest / largest vertex of the set, -1 if it is empty; the same value on every lane
GMF_DEVINL int pmc_first(const WSet& s) {
  u64 m = __ballot(s.lo != 0ull);
  if (m) {
    const int L = __ffsll((long long)m) - 1;
    const u64 w = __shfl(s.lo, L, 64);
    return L * 64 + __ffsll((long long)w) - 1;
  }
  m = __ballot(s.hi != 0ull);
  if (m) {
    const int L = __ffsll((long long)m) - 1;
    const u64 w = __shfl(s.hi, L, 64);
    return (L + 64) * 64 + __ffsll((long long)w) - 1;
  }
  return -1;
}
GMF_DEVINL int pmc_last(const WSet& s) {
  u64 m = __ballot(s.hi != 0ull);
  if (m) {
    const int L = 63 - __clzll((long long)m);
    const u64 w = __shfl(s.hi, L, 64);
    return (L + 64) * 64 + 63 - __clzll((long long)w);
  }
  m = __ballot(s.lo != 0ull);
  if (m) {
    const int L = 63 - __clzll((long long)m);
    const u64 w = __shfl(s.lo, L, 64);
    return L * 64 + 63 - __clzll((long long)w);
  }
  return -1;
}

GMF_DEVINL u64 pmc_key(int size, int vertex) { return ((u64)(unsigned)size << 32) | (u64)(0xFFFFFFFFu - (unsigned)vertex); }
GMF_DEVINL int pmc_key_size(u64 key) { return (int)(key >> 32); }
GMF_DEVINL int pmc_key_vertex(u64 key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// The greedy clique from `start`: the last candidate again and again.  At most n rounds.  `emit(k, vertex)` sees every member.
template <typename Emit>
GMF_DEVINL int pmc_greedy(const u64* __restrict__ rows, int ld, int W, int lane, int start, Emit emit) {
  WSet P = pmc_row(rows + (size_t)start * ld, W, lane);
  int size = 1;
  emit(0, start);
  for (int u; (u = pmc_last(P)) >= 0;) {
    emit(size, u);
    ++size;
    pmc_and(P, pmc_row(rows + (size_t)u * ld, W, lane));      // no diagonal: u leaves with it
  }
  return size;
}

// True iff the greedy sequential colouring of P (San Segundo's BBMC order: lowest vertex first, class by class) needs at most
// `room` colours: then no clique of P has more than `room` members.  Stops as soon as the answer is no.  At most |P| rounds.
GMF_DEVINL bool pmc_colours_within(WSet U, const u64* __restrict__ rows, int ld, int W, int lane, int room) {
  int ncol = 0;
  while (!pmc_empty(U)) {
    if (++ncol > room) return false;
    WSet Q = U;
    for (int v; (v = pmc_first(Q)) >= 0;) {
      pmc_drop(U, v, lane);
      pmc_drop(Q, v, lane);
      const WSet r = pmc_row(rows + (size_t)v * ld, W, lane);
      Q.lo &= ~r.lo;
      Q.hi &= ~r.hi;
    }
  }
  return true;
}

}  // namespace

// grid (256-row tiles of the largest pair, B), block 256.  ld: words per bit row.
__global__ void __launch_bounds__(256)
k_pmc_graph(const float* __restrict__ corr, const int* __restrict__ offsets, u64* __restrict__ bits, int* __restrict__ degree,
            long long total_rows, int max_n, int ld, float thr, int metric) {
  __shared__ float sc[256][6];
  const int pair = blockIdx.y, tid = threadIdx.x;
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n) || (int)blockIdx.x * 256 >= n) return;
  const int row = blockIdx.x * 256 + tid;
  float c[6];
  {
    const float* p = corr + (size_t)(r0 + min(row, n - 1)) * 6;
#pragma unroll
    for (int e = 0; e < 6; ++e) c[e] = p[e];
  }
  int deg = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    __syncthreads();
    {
      const int j = c0 + tid;
      const float* p = corr + (size_t)(r0 + min(j, n - 1)) * 6;
#pragma unroll
      for (int e = 0; e < 6; ++e) sc[tid][e] = p[e];
    }
    __syncthreads();
    const int words = min(4, (n - c0 + 63) / 64);
    for (int w = 0; w < words; ++w) {
      u64 word = 0ull;
#pragma unroll 8
      for (int b = 0; b < 64; ++b) {
        const float* q = sc[w * 64 + b];
        const float dx = c[0] - q[0], dy = c[1] - q[1], dz = c[2] - q[2];
        const float ex = c[3] - q[3], ey = c[4] - q[4], ez = c[5] - q[5];
        float a = (dx * dx + dy * dy) + dz * dz;
        float e = (ex * ex + ey * ey) + ez * ez;
        if (metric == kPmcLength) { a = __fsqrt_rn(a); e = __fsqrt_rn(e); }
        const int j = c0 + w * 64 + b;
        const bool edge = fabsf(a - e) < thr && j < n && j != row;
        word |= (u64)(edge ? 1 : 0) << b;
      }
      if (row < n) bits[(size_t)(r0 + row) * ld + (c0 >> 6) + w] = word;
      deg += __popcll(word);
    }
  }
  if (row < n) degree[r0 + row] = deg;
}

// grid (B), block 1024.  Peels by core level: every round removes the vertices whose remaining degree is at most the level (the
// level rises to the smallest remaining degree when it must), in row order, and takes them off their neighbours' degrees.  At most
// n rounds.  Also clears the pair's counters for the launches that follow.
__global__ void __launch_bounds__(1024)
k_pmc_order(const u64* __restrict__ bits, const int* __restrict__ degree, const int* __restrict__ offsets, int* __restrict__ order,
            u64* __restrict__ hbest, u64* __restrict__ best, u64* __restrict__ steps, int* __restrict__ next_root,
            int* __restrict__ stopped, u64* __restrict__ wave_key, long long total_rows, int max_n, int ld) {
  __shared__ int deg[kPmcMaxN];
  __shared__ u64 alive[kPmcMaxN / 64], mask[kPmcMaxN / 64];
  __shared__ int wbase[kPmcMaxN / 64];
  __shared__ int s_min, s_cnt;
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < kPmcWaves) wave_key[(size_t)pair * kPmcWaves + tid] = 0ull;
  if (tid == 0) { hbest[pair] = 0ull; best[pair] = 0ull; steps[pair] = 0ull; next_root[pair] = 0; stopped[pair] = 0; }
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n)) return;
  const int W = (n + 63) / 64;
  for (int v = tid; v < kPmcMaxN; v += 1024) deg[v] = v < n ? degree[r0 + v] : 0x7FFFFFFF;
  if (tid < kPmcMaxN / 64) {
    const int lo = tid * 64;
    alive[tid] = lo + 64 <= n ? ~0ull : (lo < n ? ((1ull << (n - lo)) - 1ull) : 0ull);
  }
  __syncthreads();
  int count = 0, level = 0;
  while (count < n) {
    if (tid == 0) s_min = 0x7FFFFFFF;
    __syncthreads();
    int m = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < kPmcMaxN / 1024; ++j) {
      const int v = j * 1024 + tid;
      if ((alive[v >> 6] >> (v & 63)) & 1ull) m = min(m, deg[v]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    if (lane == 0) atomicMin(&s_min, m);
    __syncthreads();
    level = max(level, s_min);
    unsigned flags = 0;
#pragma unroll
    for (int j = 0; j < kPmcMaxN / 1024; ++j) {
      const int v = j * 1024 + tid;      // the wave's 64 vertices are one word of the mask
      const bool f = ((alive[v >> 6] >> (v & 63)) & 1ull) && deg[v] <= level;
      const u64 b = __ballot(f);
      if (lane == 0) mask[j * 16 + wave] = b;
      flags |= (f ? 1u : 0u) << j;
    }
    __syncthreads();
    if (tid < kPmcMaxN / 64) {
      int s = 0;
      for (int j = 0; j < tid; ++j) s += __popcll(mask[j]);
      wbase[tid] = s;
      if (tid == kPmcMaxN / 64 - 1) s_cnt = s + __popcll(mask[tid]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPmcMaxN / 1024; ++j) {
      if (!((flags >> j) & 1u)) continue;
      const int v = j * 1024 + tid;
      const int p = count + wbase[v >> 6] + __popcll(mask[v >> 6] & ((1ull << (v & 63)) - 1ull));
      order[r0 + p] = v;
    }
    if (tid < kPmcMaxN / 64) alive[tid] &= ~mask[tid];
    // the removed vertices leave their neighbours' degrees: one wave per removed vertex, its row across the lanes
    int idx = 0;
    for (int j = 0; j < W; ++j) {
      for (u64 mm = mask[j]; mm; mm &= mm - 1ull, ++idx) {
        if ((idx & 15) != wave) continue;
        const u64* row = bits + (size_t)(r0 + j * 64 + __ffsll((long long)mm) - 1) * ld;
        for (int wi = lane; wi < W; wi += 64)
          for (u64 x = row[wi]; x; x &= x - 1ull) atomicSub(&deg[wi * 64 + __ffsll((long long)x) - 1], 1);
      }
    }
    __syncthreads();
    count += s_cnt;
  }
}

// grid (rows of the largest pair, B), block 128: new row p, one thread per word.
__global__ void __launch_bounds__(128)
k_pmc_renumber(const u64* __restrict__ bits, const int* __restrict__ order, const int* __restrict__ offsets, u64* __restrict__ bits2,
               long long total_rows, int max_n, int ld) {
  const int pair = blockIdx.y, p = blockIdx.x;
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n) || p >= n) return;
  const int W = (n + 63) / 64;
  const u64* row = bits + (size_t)(r0 + order[r0 + p]) * ld;
  for (int wq = threadIdx.x; wq < W; wq += 128) {
    u64 word = 0ull;
    const int cols = min(64, n - wq * 64);
    for (int b = 0; b < cols; ++b) {
      const int u = order[r0 + wq * 64 + b];
      word |= ((row[u >> 6] >> (u & 63)) & 1ull) << b;
    }
    bits2[(size_t)(r0 + p) * ld + wq] = word;
  }
}

// grid (ceil(rows of the largest pair / 4), B), block 256: one wave per start vertex.
__global__ void __launch_bounds__(256)
k_pmc_greedy(const u64* __restrict__ bits2, const int* __restrict__ offsets, u64* __restrict__ hbest, long long total_rows,
             int max_n, int ld) {
  const int pair = blockIdx.y, lane = threadIdx.x & 63, start = blockIdx.x * 4 + (threadIdx.x >> 6);
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n) || start >= n) return;
  const int size = pmc_greedy(bits2 + (size_t)r0 * ld, ld, (n + 63) / 64, lane, start, [](int, int) {});
  if (lane == 0) atomicMax(&hbest[pair], pmc_key(size, start));
}

// One 64-bit word per lane: a set over a root's own candidates, renumbered 0 .. D-1 (D <= kPmcLocal, so lanes 0..5 carry it).
GMF_DEVINL int pmc1_first(u64 x) {
  const u64 m = __ballot(x != 0ull);
  if (!m) return -1;
  const int L = __ffsll((long long)m) - 1;
  const u64 w = __shfl(x, L, 64);
  return L * 64 + __ffsll((long long)w) - 1;
}
GMF_DEVINL int pmc1_count(u64 x) {
  int c = __popcll(x);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// grid (kPmcWaves, B), block 64: one wave, roots by ticket from the last vertex down.  Every node expanded is counted first, and a
// count at the budget ends the wave: no loop here runs past the budget, and no wave waits for another.
//
// Both forms branch in vertex order - the first candidate joins, and a node's list of branches ends when the greedy colouring of
// what is left no longer passes the bar - so the tree is fixed and the bar only ends lists early.  A root with at most
// `local_rows` later neighbours (by default every root of a graph of degeneracy <= 384) is searched in LDS: its candidates are
// renumbered, their adjacency is a [D][6]-word matrix, and each level keeps its remaining candidates.  A wider root keeps no
// sets and reads the rows of the bit matrix: the candidates left at a level are the common neighbours of the clique so far behind
// the vertex tried last.  (Branching on a vertex of the last colour class instead, Tomita's rule, was tried in the LDS form: on
// the 3DMatch-shape graphs at N = 1000 one root alone then took more nodes than the whole search does in vertex order.)
__global__ void __launch_bounds__(64)
k_pmc_search(const u64* __restrict__ bits2, const int* __restrict__ offsets, const u64* __restrict__ hbest, u64* __restrict__ best,
             u64* __restrict__ steps, int* __restrict__ next_root, int* __restrict__ stopped, u64* __restrict__ wave_key,
             unsigned short* __restrict__ wave_best, long long total_rows, int max_n, int ld, u64 max_steps, int local_rows) {
  constexpr int LW = kPmcLocal / 64;
  __shared__ unsigned short R[kPmcMaxN];             // the clique so far (wide roots: vertices; local roots: local numbers from R[1])
  __shared__ unsigned short Lv[kPmcLocal];           // local number -> vertex
  __shared__ u64 adjL[kPmcLocal * LW];               // the candidates' adjacency in local numbers
  __shared__ u64 stackL[(kPmcLocal + 1) * LW];       // stackL[d]: the candidates left at the level of d members
  const int pair = blockIdx.y, lane = threadIdx.x;
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n)) return;
  const int W = (n + 63) / 64;
  const u64* rows = bits2 + (size_t)r0 * ld;
  const int h = pmc_key_size(hbest[pair]);
  const size_t slot = (size_t)pair * kPmcWaves + blockIdx.x;
  unsigned short* mine = wave_best + slot * (size_t)max_n;
  u64 my_key = 0ull;
  for (;;) {
    int root = 0;
    if (lane == 0) root = n - 1 - atomicAdd(&next_root[pair], 1);
    root = __shfl(root, 0, 64);
    if (root < 0 || __hip_atomic_load(&stopped[pair], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    int own = h, d = 1;
    bool local = false;
    // a clique of d members larger than any this root had: R[0..d) goes to the wave's list if its key is the wave's largest
    auto record = [&]() {
      own = d;
      const u64 key = pmc_key(d, root);
      if (key <= my_key) return;
      my_key = key;
      __syncthreads();      // (one wave: R's stores before the loads below)
      for (int k = lane; k < d; k += 64) mine[k] = (local && k > 0) ? Lv[R[k]] : R[k];
      if (lane == 0) {
        wave_key[slot] = key;
        atomicMax(&best[pair], key);
      }
    };
    // counts one expanded node; false: the budget has ended the search
    auto step = [&]() {
      u64 s = 0ull;
      if (lane == 0) s = atomicAdd(&steps[pair], 1ull);
      s = __shfl(s, 0, 64);
      if (s < max_steps) return true;
      if (lane == 0) __hip_atomic_store(&stopped[pair], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    };
    auto bar_now = [&]() {      // a branch that cannot pass this size is cut
      return max(own, pmc_key_size(__hip_atomic_load(&best[pair], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) - 1);
    };
    WSet P = pmc_row(rows + (size_t)root * ld, W, lane);
    P.lo &= pmc_above(lane, root);
    P.hi &= pmc_above(lane + 64, root);
    const int D = pmc_count(P);
    if (1 + D <= bar_now()) continue;
    __syncthreads();
    if (lane == 0) R[0] = (unsigned short)root;
    if (D <= local_rows) {
      local = true;
      const int Wl = (D + 63) >> 6;
      for (int k = 0; k < D; ++k) {
        const int v = pmc_first(P);
        pmc_drop(P, v, lane);
        if (lane == 0) Lv[k] = (unsigned short)v;
      }
      __syncthreads();
      int myv[LW];
#pragma unroll
      for (int w = 0; w < LW; ++w) myv[w] = w * 64 + lane < D ? (int)Lv[w * 64 + lane] : -1;
      for (int i = 0; i < D; ++i) {
        const u64* row = rows + (size_t)Lv[i] * ld;
#pragma unroll
        for (int w = 0; w < LW; ++w) {
          bool bit = false;
          if (w < Wl && myv[w] >= 0) bit = (row[myv[w] >> 6] >> (myv[w] & 63)) & 1ull;
          const u64 word = __ballot(bit);
          if (lane == 0) adjL[i * LW + w] = word;
        }
      }
      __syncthreads();
      u64 X = 0ull;      // all D candidates
      if (lane < Wl) X = (lane == Wl - 1 && (D & 63)) ? ((1ull << (D & 63)) - 1ull) : ~0ull;
      for (;;) {
        // the node (R[0..d), X)
        const int c = pmc1_count(X);
        int pick = -1;
        if (c == 0) {
          if (d > own) record();
        } else {
          const int bar = bar_now();
          if (d + c > bar) {
            if (!step()) return;
            // the greedy colouring of pmc_colours_within on the local matrix: cut iff it needs at most bar - d colours
            int ncol = 0;
            bool within = true;
            for (u64 U = X; within && __ballot(U != 0ull);) {
              if (++ncol > bar - d) { within = false; break; }
              u64 Q = U;
              for (int v; (v = pmc1_first(Q)) >= 0;) {
                const u64 keep = (v >> 6) == lane ? ~(1ull << (v & 63)) : ~0ull;
                U &= keep;
                Q &= keep & ~(lane < LW ? adjL[v * LW + lane] : 0ull);
              }
            }
            if (!within) pick = pmc1_first(X);      // the first candidate joins; the others are all behind it
          }
        }
        if (pick >= 0) {      // down: `pick` joins, and leaves the level's candidates
          if ((pick >> 6) == lane) X &= ~(1ull << (pick & 63));
          if (lane < LW) stackL[d * LW + lane] = X;
          if (lane == 0) R[d] = (unsigned short)pick;
          X &= lane < LW ? adjL[pick * LW + lane] : 0ull;
          ++d;
          continue;
        }
        if (d == 1) break;
        --d;
        X = lane < LW ? stackL[d * LW + lane] : 0ull;
      }
      continue;
    }
    for (;;) {
      // the node (R[0..d), P)
      const int c = pmc_count(P);
      bool cut = true;
      if (c == 0) {
        if (d > own) record();
      } else {
        const int bar = bar_now();
        if (d + c > bar) {
          if (!step()) return;
          cut = pmc_colours_within(P, rows, ld, W, lane, bar - d);
        }
      }
      if (!cut) {      // down: the first candidate joins; the others are all behind it
        const int v = pmc_first(P);
        if (lane == 0) R[d] = (unsigned short)v;
        ++d;
        pmc_and(P, pmc_row(rows + (size_t)v * ld, W, lane));
        continue;
      }
      // back: the last member leaves, and what is left at its level are the common neighbours of the others behind it
      if (d == 1) break;
      --d;
      __syncthreads();
      const int v = R[d];
      P.lo = pmc_above(lane, v);
      P.hi = pmc_above(lane + 64, v);
      for (int k0 = 0; k0 < d; k0 += 64) {
        const int mem = k0 + lane < d ? (int)R[k0 + lane] : 0;
        const int cnt = min(64, d - k0);
        int k = 0;
        for (; k + 4 <= cnt; k += 4) {      // four rows in flight
          const WSet a = pmc_row(rows + (size_t)__shfl(mem, k, 64) * ld, W, lane);
          const WSet b = pmc_row(rows + (size_t)__shfl(mem, k + 1, 64) * ld, W, lane);
          const WSet e = pmc_row(rows + (size_t)__shfl(mem, k + 2, 64) * ld, W, lane);
          const WSet f = pmc_row(rows + (size_t)__shfl(mem, k + 3, 64) * ld, W, lane);
          P.lo &= (a.lo & b.lo) & (e.lo & f.lo);
          P.hi &= (a.hi & b.hi) & (e.hi & f.hi);
        }
        for (; k < cnt; ++k) pmc_and(P, pmc_row(rows + (size_t)__shfl(mem, k, 64) * ld, W, lane));
      }
    }
  }
}

// grid (B), block 256.  The winner: the search's incumbent where it is larger than the starting clique, else the starting clique
// (replayed from its start vertex by wave 0).  A pair beyond the caller's bounds gets zeros.
__global__ void __launch_bounds__(256)
k_pmc_finish(const u64* __restrict__ bits2, const int* __restrict__ order, const int* __restrict__ offsets,
             const u64* __restrict__ hbest, const u64* __restrict__ best, const u64* __restrict__ steps,
             const int* __restrict__ stopped, const u64* __restrict__ wave_key, const unsigned short* __restrict__ wave_best,
             float* __restrict__ labels, int* __restrict__ size_out, int* __restrict__ exact_out, long long* __restrict__ steps_out,
             int* __restrict__ degree, long long total_rows, int max_n, int ld) {
  __shared__ int s_slot;
  const int pair = blockIdx.x, tid = threadIdx.x;
  int r0, n;
  if (!pmc_pair(offsets, pair, total_rows, max_n, r0, n)) {
    if (n > 0 && r0 >= 0 && (long long)offsets[pair + 1] <= total_rows)      // too long for the call's bound: zeros
      for (int i = tid; i < n; i += 256) { labels[r0 + i] = 0.f; degree[r0 + i] = 0; }
    if (tid == 0) { size_out[pair] = 0; exact_out[pair] = n == 0 ? 1 : 0; steps_out[pair] = 0; }
    return;
  }
  for (int i = tid; i < n; i += 256) labels[r0 + i] = 0.f;
  const u64 hk = hbest[pair], bk = best[pair];
  if (tid == 0) s_slot = -1;
  __syncthreads();      // (also: the zeros above are written before the ones below)
  if (pmc_key_size(bk) > pmc_key_size(hk)) {
    if (tid < kPmcWaves && wave_key[(size_t)pair * kPmcWaves + tid] == bk) s_slot = tid;
    __syncthreads();
    if (s_slot >= 0) {
      const unsigned short* mem = wave_best + ((size_t)pair * kPmcWaves + s_slot) * (size_t)max_n;
      for (int k = tid; k < pmc_key_size(bk); k += 256) labels[r0 + order[r0 + mem[k]]] = 1.f;
    }
    if (tid == 0) size_out[pair] = pmc_key_size(bk);
  } else {
    if (tid < 64)
      pmc_greedy(bits2 + (size_t)r0 * ld, ld, (n + 63) / 64, tid, pmc_key_vertex(hk),
                 [&](int, int v) { if (tid == 0) labels[r0 + order[r0 + v]] = 1.f; });
    if (tid == 0) size_out[pair] = pmc_key_size(hk);
  }
  if (tid == 0) {
    exact_out[pair] = stopped[pair] ? 0 : 1;
    steps_out[pair] = (long long)steps[pair];
  }
}

hipError_t launch_pmc_graph(const float* corr, const int* offsets, int B, long long total_rows, int max_n, float threshold,
                            int metric, u64* bits, int* degree, hipStream_t s) {
  if (max_n <= 0 || total_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pmc_graph, dim3((max_n + 255) / 256, B), dim3(256), 0, s, corr, offsets, bits, degree, total_rows, max_n,
                     pmc_row_words(max_n), threshold, metric);
  return hipGetLastError();
}

hipError_t launch_max_clique(const float* corr, const float* src, const float* tgt, const int* offsets, int B, long long total_rows,
                             int max_n, float threshold, int metric, long long max_steps, int local_rows, const PmcScratch& ws,
                             float* labels, float* T_out, int* size_out, int* exact_out, long long* steps_out, int* degree_out, hipStream_t s) {
  const int ld = pmc_row_words(max_n);
  if (max_n > 0 && total_rows > 0) {
    hipLaunchKernelGGL(k_pmc_graph, dim3((max_n + 255) / 256, B), dim3(256), 0, s, corr, offsets, ws.bits, degree_out, total_rows,
                       max_n, ld, threshold, metric);
    hipLaunchKernelGGL(k_pmc_order, dim3(B), dim3(1024), 0, s, ws.bits, degree_out, offsets, ws.order, ws.hbest, ws.best, ws.steps,
                       ws.next_root, ws.stopped, ws.wave_key, total_rows, max_n, ld);
    hipLaunchKernelGGL(k_pmc_renumber, dim3(max_n, B), dim3(128), 0, s, ws.bits, ws.order, offsets, ws.bits2, total_rows, max_n, ld);
    hipLaunchKernelGGL(k_pmc_greedy, dim3((max_n + 3) / 4, B), dim3(256), 0, s, ws.bits2, offsets, ws.hbest, total_rows, max_n, ld);
    hipLaunchKernelGGL(k_pmc_search, dim3(kPmcWaves, B), dim3(64), 0, s, ws.bits2, offsets, ws.hbest, ws.best, ws.steps,
                       ws.next_root, ws.stopped, ws.wave_key, ws.wave_best, total_rows, max_n, ld, (u64)max_steps,
                       local_rows < kPmcLocal ? local_rows : kPmcLocal);
  }
  // (with no rows at all the scratch is empty and every pair is: k_pmc_finish reads none of it then)
  hipLaunchKernelGGL(k_pmc_finish, dim3(B), dim3(256), 0, s, ws.bits2, ws.order, offsets, ws.hbest, ws.best, ws.steps, ws.stopped,
                     ws.wave_key, ws.wave_best, labels, size_out, exact_out, steps_out, degree_out, total_rows, max_n, ld);
  return launch_sm_pose(src, tgt, labels, labels, offsets, B, total_rows, max_n, T_out, s);
}

}  // namespace gmf
