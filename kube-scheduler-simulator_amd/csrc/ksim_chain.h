// ksim_chain.h — the batch paths' greedy chain, run inside the chain + pairs
// launches of the P100, ADAPT and topology batches.
#pragma once
#include "ksim_device.h"
#include "ksim_internal.h"
#include "ksim_wave.h"

namespace ksim {

constexpr int kHashBits = kBatchPods * kTopT <= 2048 ? 12 : kBatchPods * kTopT <= 4096 ? 13 : 14;
constexpr int kHashSlots = 1 << kHashBits;     // >= 2 x the list entries (linear probing)
constexpr int kChainRounds = 64;               // exact prefix kept if not converged by then

// KSIM_CHAIN_DELAY builds (the race regression test, tests/test_gpu_chain_race.py):
// stretch the two windows the round tags and the per-parity tables protect.
// A middle wave sleeps right after the round's barrier, before it reads the
// round's table and the previous round's flag, so the faster waves have
// registered for the next round by then; the last wave sleeps before it
// registers for the next round, so it arrives last at every barrier and the
// others wait a whole sleep between their reads and its writes.  s_sleep is a
// scalar ALU wait.
#ifdef KSIM_CHAIN_DELAY
#define CHAIN_DELAY(wave_sel)                                                      \
  do {                                                                             \
    if ((int)(threadIdx.x >> 6) == (wave_sel)) {                                   \
      __builtin_amdgcn_s_sleep(127);                                               \
      __builtin_amdgcn_s_sleep(127);                                               \
    }                                                                              \
  } while (0)
#else
#define CHAIN_DELAY(wave_sel) do {} while (0)
#endif
static_assert(kBatchPods * kTopT * 2 <= kHashSlots, "chain hash table too small");

// Clusters of at most kChainDirect nodes index the holders by node id (no hash
// probes while the lists are registered): config 2 7.03 -> 6.80 ms per step
// (profiles/r03/ab_chaindirect)
constexpr int kChainDirect = 8192;
constexpr int kChainHoldSlots = kHashSlots > kChainDirect ? kHashSlots : kChainDirect;
struct ChainLds {
  int32_t key[kHashSlots];                     // node id in the slot, -1 = empty (hash mode)
  int32_t hold[2][kChainHoldSlots];            // per round parity: (round tag << 9) | (511 - lowest pod holding the slot)
  int16_t rep[kBatchPods][kTopT];              // slot of each list entry
  int32_t first[2], cut;                      // first: per round parity, (round tag << 9) | (511 - first changed pod)
};

// The chain of one batch in one block of kBatchPods threads (thread i = pod
// i; pods from nb_cap on take no part).  Returns false when the batch is empty (block-uniform); else *gk = pod
// i's guessed key (0: none, or i past the exact prefix) and *nchain = the
// prefix length.  A pure function of the lists: every block that runs it gets
// the same guesses.
// The top T of two descending lists, descending, into x: the elementwise max
// of x and y reversed is bitonic and holds the top T; a half-cleaner network
// sorts it.
__device__ __forceinline__ void merge_top(uint64_t (&x)[kTopT], const uint64_t (&y)[kTopT]) {
  static_assert((kTopT & (kTopT - 1)) == 0, "bitonic merge: T a power of two");
#pragma unroll
  for (int e = 0; e < kTopT; e++) x[e] = umax64(x[e], y[kTopT - 1 - e]);
#pragma unroll
  for (int h = kTopT / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int e = 0; e < kTopT; e++)
      if ((e & h) == 0) cswap_desc(x[e], x[e + h]);
}

// R > 1: pod i's list is R records (i * R + r: a node slice's provable top-T,
// count, complete), merged here.  A key is provable when it is >= the last
// listed key of every incomplete record (a record hides only keys below its
// last); the merged list is complete when every record is and nothing was
// dropped.
template <int R = 1>
__device__ __forceinline__ bool chain_block(ChainLds& L, const DevState* __restrict__ st,
                                            const uint64_t* __restrict__ topk,
                                            const int32_t* __restrict__ topk_cnt,
                                            const int32_t* __restrict__ topk_complete, uint64_t* gk,
                                            int32_t* nchain_out, unsigned long long* __restrict__ dbg,
                                            int32_t nb_cap = kBatchPods, int32_t direct_n = 0) {
  int32_t* const s_key = L.key;
  int32_t& s_cut = L.cut;
  // phase clock (100 MHz realtime): dbg[0] setup, dbg[1] rounds, dbg[2] epilogue, dbg[3] launches,
  // dbg[4] passes of the round loop (with the lagging check)
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const int i = threadIdx.x;                   // one pod per thread
  // the pod's list, count and state in flight together (independent loads;
  // the buffers hold kBatchPods entries, so no bound check is needed yet)
  uint64_t lst[kTopT];
  int cnt0, complete0;
  if constexpr (R == 1) {
#pragma unroll
    for (int e = 0; e < kTopT; e++) lst[e] = topk[(size_t)i * kTopT + e];
    cnt0 = topk_cnt[i];
    complete0 = topk_complete[i];
  } else {
    uint64_t k[R][kTopT];
    int32_t rc[R], rp[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int e = 0; e < kTopT; e++) k[r][e] = topk[((size_t)i * R + r) * kTopT + e];
      rc[r] = topk_cnt[i * R + r];
      rp[r] = topk_complete[i * R + r];
    }
    uint64_t thr = 0;
    int32_t all_c = 1, csum = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
      uint64_t last = ~0ull;                     // an incomplete empty record proves nothing
#pragma unroll
      for (int e = 0; e < kTopT; e++) last = e == rc[r] - 1 ? k[r][e] : last;
      if (!rp[r]) thr = umax64(thr, last);
      all_c &= rp[r];
      csum += rc[r];
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int e = 0; e < kTopT; e++)
        if (k[r][e] < thr) k[r][e] = 0;          // a sorted suffix: the records stay sorted
#pragma unroll
    for (int e = 0; e < kTopT; e++) lst[e] = k[0][e];
#pragma unroll
    for (int r = 1; r < R; r++) merge_top(lst, k[r]);
    cnt0 = 0;
#pragma unroll
    for (int e = 0; e < kTopT; e++) cnt0 += lst[e] != 0;
    complete0 = all_c && csum <= kTopT;
  }
  const int32_t base = st->cursor;
  const int32_t nb = min(nb_cap, st->end - base);   // nb_cap: the topology batch's pod count
  if (nb <= 0) return false;
  const int cnt = i < nb ? cnt0 : 0;
  const bool incomplete = i < nb && !complete0;
  if (i < 2) L.first[i] = 0;                   // tag 0: no round's flag
  if (i == 0) s_cut = kBatchPods;              // lowered after the rounds (the epilogue)
  // this pod's slots in registers (selects below, never a dynamic index)
  int32_t rep[kTopT];
  if (direct_n > 0 && direct_n <= kChainDirect) {   // block-uniform: the slot is the node id
#pragma unroll
    for (int e = 0; e < kTopT; e++) rep[e] = e < cnt ? key_node(lst[e]) : -1;
  } else {
    for (int x = i; x < kHashSlots; x += kBatchPods) s_key[x] = -1;
    lds_barrier();
#pragma unroll
    for (int e = 0; e < kTopT; e++) {
      int16_t slot = -1;
      if (e < cnt) {
        const int32_t node = key_node(lst[e]);
        uint32_t h = ((uint32_t)node * 2654435761u) >> (32 - kHashBits);
        while (true) {
          const int32_t prev = atomicCAS(&s_key[h], -1, node);
          if (prev == -1 || prev == node) break;
          h = (h + 1) & (kHashSlots - 1);
        }
        slot = (int16_t)h;
      }
      L.rep[i][e] = slot;
    }
    lds_barrier();
#pragma unroll
    for (int e = 0; e < kTopT; e++) rep[e] = L.rep[i][e];
  }
  // only the slots the lists name are ever read: each pod clears its own (a
  // slot shared by several lists is cleared by each, to the same value), once:
  // tag 0 is older than every round's
#pragma unroll
  for (int e = 0; e < kTopT; e++)
    if (e < cnt) L.hold[0][rep[e]] = L.hold[1][rep[e]] = 0;
  lds_barrier();
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  int a = cnt > 0 ? 0 : -1;                    // current guess (entry index) or -1
  int first = kBatchPods, rounds = 0;
  // Round r has parity r & 1 and tag r + 1.  It registers (tag << 9) | (511 -
  // pod) in hold[r & 1] by atomicMax, so the lowest pod of the newest round
  // wins and a word of an older round (or the setup's 0) reads as empty: no
  // slot and no flag is ever reset, and a round is one barrier B(r):
  //   hold[par]  written in round r before B(r); read between B(r) and the
  //              thread's arrival at B(r + 1); next written in round r + 2,
  //              after B(r + 1).
  //   first[par] written between B(r) and B(r + 1); read between B(r + 1) and
  //              B(r + 2); next written in round r + 2, after B(r + 2).
  // One table for both parities would not do: a fast wave's round r + 1
  // registration would overwrite what a slow wave still reads in round r.
  // The convergence test lags a round (round r reads round r - 1's flag in the
  // same wait as its table reads), so a launch runs one more registration and
  // barrier than it has rounds; at the cap the last pass is the barrier and
  // the flag read alone, and first is round kChainRounds - 1's.
  static_assert(kBatchPods <= 512, "chain words: 9 bits of pod under the round tag");
  for (;; rounds++) {
    const int par = rounds & 1;
    const int32_t mine = ((rounds + 1) << 9) | (511 - i);
    int32_t ra = 0;
#pragma unroll
    for (int e = 0; e < kTopT; e++) ra = e == a ? rep[e] : ra;
    if (rounds < kChainRounds && a >= 0) atomicMax(&L.hold[par][ra], mine);
    lds_barrier();
    CHAIN_DELAY(1);                            // a middle wave late after the barrier
    // the previous round's flag and every entry's holder in one wait
    const int32_t flag = L.first[par ^ 1];
    int32_t held[kTopT];
#pragma unroll
    for (int e = 0; e < kTopT; e++) held[e] = e < cnt ? L.hold[par][rep[e]] : 0;
    if (rounds >= 1) {
      const bool changed = flag >= (rounds << 9);   // round r - 1's tag: some pod changed then
      first = changed ? 511 - (flag & 511) : kBatchPods;
      if (!changed || rounds == kChainRounds) break;   // a fixpoint (every pod exact), or the cap
    }
    // the first entry not held by an earlier pod in this round
    int na = -1;
#pragma unroll
    for (int e = kTopT - 1; e >= 0; e--)
      if (e < cnt && held[e] <= mine) na = e;
    {                                          // the wave's first changed pod: one LDS atomic per wave
      const uint64_t chg = __ballot(na != a);
      if (chg && (threadIdx.x & 63) == 0)
        atomicMax(&L.first[par], ((rounds + 1) << 9) | (511 - ((int)(threadIdx.x & ~63u) + __builtin_ctzll(chg))));
    }
    a = na;
    CHAIN_DELAY((int)(blockDim.x >> 6) - 1);   // the last wave registers late
  }
  // exact prefix [0, first); an exhausted incomplete list inside it cuts the chain
  block_first_min(&s_cut, i < first && i < nb && a < 0 && incomplete);
  lds_barrier();
  const int32_t nchain = min(s_cut, min(first, nb));
  const uint64_t t2 = __builtin_amdgcn_s_memrealtime();
  uint64_t ga = 0;
#pragma unroll
  for (int e = 0; e < kTopT; e++) ga = e == a ? lst[e] : ga;   // register select, no dynamic index
  *gk = (i < nchain && a >= 0) ? ga : 0;
  *nchain_out = nchain;
  if (i == 0 && dbg) {
    const uint64_t t3 = __builtin_amdgcn_s_memrealtime();
    atomicAdd(&dbg[0], (unsigned long long)(t1 - t0));
    atomicAdd(&dbg[1], (unsigned long long)(t2 - t1));
    atomicAdd(&dbg[2], (unsigned long long)(t3 - t2));
    atomicAdd(&dbg[3], 1ull);
    atomicAdd(&dbg[4], (unsigned long long)(rounds + 1));
  }
  return true;
}

}  // namespace ksim
