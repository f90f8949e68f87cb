// lis_chain.h -- what the block-parallel list kernels of the decoder (k_lis_l0, k_lis_l1, k_lis_l2: speck_dec.hip)
// have in common.  Device code only.
//
// A list of the sorting pass is a run of tokens in the stream, one per entry: '0' (the entry stays in the list), or
// '1' followed by the split of its set.  Where a token starts is known only once the one before it is decoded, so
// the stream is cut into blocks of W bit positions that a ticket counter hands out in order, and a block works
// speculatively.  Each phase below is one function; a kernel calls them in this order with its own parts in between:
//
//   chain_ticket       take the next block (none once the list's last entry is decoded or the flag words run out)
//   chain_load_words   the block's stream words, and as many more as a token can reach past it, into LDS
//   (the kernel)       its class tables: U[r] = length of the token that would start at position r, for every r
//   chain_hops         by pointer jumping, for every r: where a chain of tokens entering at r leaves its 64-position
//                      sub-block, how many tokens it holds and how many are significant (hop64) -- a summary word,
//                      tokens << 21 | significant << 14 | position reached -- and a copy widened to 1024 positions (hopW)
//   chain_through      (the kernel's memo: the same for the whole block, for each offset a chain can enter it at)
//   lookback_wait      the predecessor's look-back word: entry offset, entries and significant entries so far
//   lookback_publish   this block's word, straight from the memo; the entry state goes to ChainShared
//   chain_entries      where the real chain enters each 1024-block, then each sub-block
//   chain_marks        the tokens really on the chain, marked in hopW with their rank:
//                      (1 + entries before the token) | significant entries before it << 16, block-local
//   chain_sweep_list   (k_lis_l1, k_lis_l2) insignificant entries go to the next list in order, significant ones park
//                      their list entry in hop64 and queue up
//
// A block is handed out only after all earlier ones, so a waiting block always waits for a workgroup that is running
// (or has seen the pass end).  A wait also ends when the pass's end marker is set, and after a minute of wall time
// (LookBackWait, lis_region.h: DecState::error = kErrLookBackTimeout).
#ifndef SPERR_AMD_LIS_CHAIN_H
#define SPERR_AMD_LIS_CHAIN_H

#include "speck_dec.h"
#include "lis_token.h"

namespace sperrhip {

constexpr uint32_t kL0None = 0xffffffffu;

// the LDS words of the skeleton: a `__shared__ ChainShared<W>` of the kernel
template <int W>
struct ChainShared {
  uint32_t entR[W / 1024], entK[W / 1024], entS[W / 1024];   // the chain where it enters a 1024-block: position, rank, significant
  uint32_t blkE[W / 64], blkK[W / 64], blkS[W / 64];         // ... and a sub-block
  uint32_t ticket;
  uint32_t e, rank, sig;     // the state the chain enters the block with
  uint32_t last, stop;       // the list ends inside this block; it ended before it (or the pass was given up)
  uint32_t endpos, endsig;   // of the last block: position after the list's last token, significant entries up to it
};

// one step along a chain of summary words
__device__ __forceinline__ uint32_t chain_step(uint32_t v, uint32_t& cnt, uint32_t& sg)
{
  cnt += v >> 21;
  sg += (v >> 14) & 0x7fu;
  return v & 0x3fffu;
}

template <int W>
__device__ __forceinline__ uint32_t chain_ticket(ChainShared<W>& cs, int32_t* planeP1, uint32_t* ticket, int p, size_t flagStride)
{
  if (threadIdx.x == 0) {
    const bool over = __hip_atomic_load(planeP1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p + 1;
    cs.ticket = over ? kL0None : atomicAdd(ticket, 1u);
  }
  __syncthreads();
  const uint32_t i = cs.ticket;
  return (i == kL0None || (size_t)i + 1 >= flagStride) ? kL0None : i;
}

// WORDS stream words from the one that holds bit `a`; words past the stream's end read as zero
template <int WORDS, int THREADS>
__device__ __forceinline__ LdsBits chain_load_words(uint64_t* wbits, const uint64_t* words, uint64_t a, uint64_t nwordsAvail)
{
  const uint64_t w0 = a >> 6;
  for (uint32_t k = threadIdx.x; k < (uint32_t)WORDS; k += THREADS)
    wbits[k] = w0 + k < nwordsAvail ? words[w0 + k] : 0ull;
  __syncthreads();
  return LdsBits{reinterpret_cast<const uint32_t*>(wbits), (uint32_t)(a & 63)};
}

template <int W, int THREADS, typename TU>
__device__ __forceinline__ void chain_hops(const LdsBits& bits, const TU* U, uint32_t* hop64, uint32_t* hopW)
{
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // chains inside 64-position sub-blocks (lane = position)
  for (uint32_t sb = wave; sb < (uint32_t)(W / 64); sb += THREADS / 64) {
    const uint32_t r = sb * 64 + lane, hEnd = (sb + 1) * 64;
    uint32_t v = (1u << 21) | (bits.bit_at(r) << 14) | (r + U[r]);
    bool inb = (v & 0x3fffu) < hEnd;
    for (int it = 0; it < 6 && __any(inb); it++) {
      const uint32_t o = __shfl(v, (v & 0x3fffu) & 63u, 64);
      if (inb) {
        v = (v & ~0x3fffu) + o;
        inb = (v & 0x3fffu) < hEnd;
      }
    }
    hop64[r] = v;
    hopW[r] = v;
  }
  __syncthreads();
  // widen a copy to 1024-position blocks (in place: any version read is a valid summary)
  for (uint32_t wide = 128; wide <= 1024; wide <<= 1) {
    for (uint32_t r = tid; r < (uint32_t)W; r += THREADS) {
      const uint32_t v = hopW[r], e = v & 0x3fffu;
      if (e < (uint32_t)W && e / wide == r / wide)
        hopW[r] = (v & ~0x3fffu) + hopW[e];
    }
    __syncthreads();
  }
}

// the whole block for a chain that enters at offset r: where it leaves (relative to the block's end), its tokens
// and its significant tokens
template <int W>
__device__ __forceinline__ uint32_t chain_through(const uint32_t* hopW, uint32_t r, uint32_t& cnt, uint32_t& sg)
{
  cnt = 0;
  sg = 0;
  while (r < (uint32_t)W)
    r = chain_step(hopW[r], cnt, sg);
  return r - W;
}

// One-word look-back: tag (plane + 1) << 56 | list ended << 55 | exit offset << XS | entries << RS | significant.
// One thread waits for the word of the block before; true: the list ended there, or the pass is over.
template <int XS, int RS>
__device__ __forceinline__ bool lookback_wait(DecState& s, int32_t* planeP1, const unsigned long long* prev, int p, uint32_t& e,
                                              uint32_t& rank, uint32_t& sg)
{
  unsigned long long f = 0;
  LookBackWait wait;
  for (;;) {
    f = __hip_atomic_load(prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((f >> 56) == (unsigned long long)(p + 1))
      break;
    // (no sleep between polls: the rest of the workgroup stands at the barrier behind this wait)
    const WaitStep ws = wait.step(planeP1, p, false);
    if (ws == kWaitOn)
      continue;
    if (ws == kWaitExpired)
      lookback_give_up(&s.error, planeP1, p);
    return true;
  }
  if ((f >> 55) & 1ull)
    return true;
  e = (uint32_t)(f >> XS) & ((1u << (55 - XS)) - 1u);
  rank = (uint32_t)(f >> RS) & ((1u << (XS - RS)) - 1u);
  sg = (uint32_t)f & ((1u << RS) - 1u);
  return false;
}

// One thread, with the entry state (e, rank, sg) it has found and the memo of offset e (exit offset, entries,
// significant entries): publishes the block's word -- or that the list ends here, which ends the pass -- and
// leaves the entry state in cs.
template <int XS, int RS, int W>
__device__ __forceinline__ void lookback_publish(ChainShared<W>& cs, int32_t* planeP1, unsigned long long* mine, int p, uint32_t n,
                                                 bool stop, uint32_t e, uint32_t rank, uint32_t sg, uint32_t mx, uint32_t mc,
                                                 uint32_t ms)
{
  const unsigned long long tag = (unsigned long long)(p + 1) << 56;
  uint32_t last = 0;
  if (!stop) {
    if (rank + mc >= n) {   // the list ends inside this block
      last = 1;
      __hip_atomic_store(mine, tag | (1ull << 55), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(planeP1, p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    else
      __hip_atomic_store(mine,
                         tag | ((unsigned long long)mx << XS) | ((unsigned long long)(rank + mc) << RS) |
                             (unsigned long long)(sg + ms),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  cs.e = e;
  cs.rank = rank;
  cs.sig = sg;
  cs.last = last;
  cs.stop = stop;
  cs.endpos = 0;
  cs.endsig = 0;
}

// (every thread, before the barrier that makes the look-back's result visible)
template <int W, int THREADS>
__device__ __forceinline__ void chain_clear_entries(ChainShared<W>& cs)
{
  for (uint32_t k = threadIdx.x; k < (uint32_t)(W / 64); k += THREADS)
    cs.blkE[k] = kL0None;
  if (threadIdx.x < W / 1024)
    cs.entR[threadIdx.x] = kL0None;
}

template <int W>
__device__ __forceinline__ void chain_entries(ChainShared<W>& cs, const uint32_t* hop64, const uint32_t* hopW)
{
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    uint32_t r = cs.e, rk = 0, sg = 0;
    while (r < (uint32_t)W) {
      cs.entR[r >> 10] = r;
      cs.entK[r >> 10] = rk;
      cs.entS[r >> 10] = sg;
      r = chain_step(hopW[r], rk, sg);
    }
  }
  __syncthreads();
  if (tid < W / 1024 && cs.entR[tid] != kL0None) {
    uint32_t r = cs.entR[tid], rk = cs.entK[tid], sg = cs.entS[tid];
    const uint32_t end = (tid + 1) * 1024;
    while (r < end) {
      cs.blkE[r >> 6] = r;
      cs.blkK[r >> 6] = rk;
      cs.blkS[r >> 6] = sg;
      r = chain_step(hop64[r], rk, sg);
    }
  }
  __syncthreads();
}

// nloc: entries the list still holds at the start of the block.  (The caller's barrier ends the phase.)
template <int W, int THREADS, typename TU>
__device__ __forceinline__ void chain_marks(ChainShared<W>& cs, const LdsBits& bits, const TU* U, uint32_t* hopW, uint32_t nloc)
{
  const uint32_t tid = threadIdx.x;
  for (uint32_t r = tid; r < (uint32_t)W; r += THREADS)
    hopW[r] = 0;
  __syncthreads();
  if (tid < W / 64 && cs.blkE[tid] != kL0None) {
    uint32_t r = cs.blkE[tid], rk = cs.blkK[tid], sg = cs.blkS[tid];
    const uint32_t end = (tid + 1) * 64;
    bool did = false;
    while (r < end && rk < nloc) {
      hopW[r] = (rk + 1u) | (sg << 16);
      rk++;
      sg += bits.bit_at(r);
      r += U[r];
      did = true;
    }
    if (did && rk == nloc) {   // this thread decoded the list's last entry
      cs.endpos = r;
      cs.endsig = sg;
    }
  }
}

// The first sweep of k_lis_l1 / k_lis_l2: insignificant entries stay; significant ones leave their list entry in
// their own words of hop64 (a significant token is 16 bits and more) and queue up in tokQ (CAP entries; *ntok counts
// on past it).  The list entries of a thread's positions are loaded before any is used.
template <int W, int THREADS, int CAP>
__device__ __forceinline__ void chain_sweep_list(const ChainShared<W>& cs, const LdsBits& bits, const uint64_t* list, uint64_t* keep,
                                                 uint32_t* hop64, const uint32_t* hopW, uint16_t* tokQ, uint32_t* ntok)
{
  constexpr int PER = W / THREADS;
  const uint32_t tid = threadIdx.x, rank0 = cs.rank, sig0 = cs.sig;
  uint32_t mk4[PER];
  uint64_t id4[PER];
#pragma unroll
  for (int j = 0; j < PER; j++)
    mk4[j] = hopW[tid + (uint32_t)j * THREADS];
#pragma unroll
  for (int j = 0; j < PER; j++)
    id4[j] = mk4[j] ? list[rank0 + (mk4[j] & 0xffffu) - 1u] : 0ull;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const uint32_t r = tid + (uint32_t)j * THREADS;
    const uint32_t mk = mk4[j];
    if (mk == 0)
      continue;
    const uint32_t q = rank0 + (mk & 0xffffu) - 1u, sb = sig0 + (mk >> 16);
    const uint64_t ident = id4[j];
    if (!bits.bit_at(r)) {
      keep[q - sb] = ident;
      continue;
    }
    hop64[r + 1] = (uint32_t)ident;
    hop64[r + 2] = (uint32_t)(ident >> 32);
    const uint32_t ti = atomicAdd(ntok, 1u);
    if (ti < (uint32_t)CAP)
      tokQ[ti] = (uint16_t)r;
  }
}

}  // namespace sperrhip

#endif
