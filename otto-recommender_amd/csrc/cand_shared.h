// Shared by candidates.hip (candidate rows) and features.hip (ranker feature columns): the source-list
// and kept-aid records, the per-aid merged source lists (k_ml_build) and their host-side construction.
// Each including translation unit compiles its own copy of the kernels (internal linkage).
#pragma once
#include <algorithm>
#include "prims.h"
#include "table.h"

namespace ottohip {

constexpr int CS_MAXE = 512;      // events per session handled by k_cand_aids
constexpr int CS_SRC = 7;         // 5 co-count lists + 2 kNN lists
constexpr int CS_NLAST = 99;      // RETRIEVE_N_LAST_* / RETRIEVE_N_MOST_FREQUENT (config.py:76-79)
constexpr uint32_t CS_EMPTY = 0xFFFFFFFFu;

struct CandLists {
  const uint32_t* off[CS_SRC];   // per source: [n_items + 1] offsets into nxt / rank (by aid)
  const int32_t* nxt[CS_SRC];
  const int16_t* rank[CS_SRC];
  int32_t n_items;
  const uint32_t* pop_off;       // [n_clusters + 1]
  const int32_t* pop_aid;
  int32_t n_clusters;
};

// kept aid record: aid, info = ts_order_aid (16 b) | type mask << 16 (3 b) | th << 19 (5 b)
struct KeptAid { int32_t aid; uint32_t info; };

__device__ __forceinline__ bool rank_before(int ka, int32_t aa, int kb, int32_t ab) {  // desc key, asc aid
  return ka > kb || (ka == kb && aa < ab);
}

// Per-aid union of the 7 source lists (SURVEY.md §8(a) R4-R5 are pair-level: a pair (aid, aid_next)
// carries every source that lists it and is kept if its best rank passes). One wave per aid:
// elements (x, source bit, rank) of all lists in LDS, duplicates of x folded (OR of bits, min rank).
// A kept aid's trim threshold th is at most 31 (5 bits) and R5 keeps an entry iff x == aid or its rank
// <= th, so the unique entries are written ordered by that test: the self entry (x == aid) first, then by
// rank 0..31 (entries ranked above 31 can never be kept and are dropped); ucnt[a] = entries written and
// pc[a][th] = the entries a kept aid with threshold th takes (a prefix of the list): k_cand_build scans
// only those instead of every entry (the long sessions' lists were mostly entries above their th).
constexpr int ML_MAX = 256;  // elements per aid across the 7 lists
constexpr int ML_TH = 32;    // trim thresholds 0..31
static __global__ __launch_bounds__(256) void k_ml_build(CandLists L, const uint32_t* __restrict__ eoff,
                                                         int32_t* __restrict__ mx, uint16_t* __restrict__ mbr,
                                                         uint32_t* __restrict__ ucnt, uint16_t* __restrict__ pc,
                                                         int* __restrict__ err) {
  __shared__ uint32_t ex[4][ML_MAX];
  __shared__ uint16_t eb[4][ML_MAX], uk[4][ML_MAX];
  __shared__ uint32_t hs[4][ML_TH + 1];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int64_t a = (int64_t)blockIdx.x * 4 + w;
  if (a >= L.n_items) return;
  uint32_t beg[CS_SRC], len[CS_SRC], tot = 0;
#pragma unroll
  for (int q = 0; q < CS_SRC; ++q) {
    if (L.off[q]) { beg[q] = L.off[q][a]; len[q] = L.off[q][a + 1] - beg[q]; } else { beg[q] = 0; len[q] = 0; }
    tot += len[q];
  }
  if (tot > ML_MAX) {
    if (l == 0) { atomicOr(err, 4); ucnt[a] = 0; }
    if (l < ML_TH) pc[a * ML_TH + l] = 0;
    return;
  }
  if (l <= ML_TH) hs[w][l] = 0;
  for (uint32_t e = l; e < tot; e += 64) {
    uint32_t j = e;
    int q = 0;
#pragma unroll
    for (int z = 0; z < CS_SRC; ++z)
      if (q == z && j >= len[z]) { j -= len[z]; q = z + 1; }
    const int32_t* np = L.nxt[0];
    const int16_t* rp = L.rank[0];
    uint32_t b0 = beg[0];
#pragma unroll
    for (int z = 1; z < CS_SRC; ++z)
      if (q == z) { np = L.nxt[z]; rp = L.rank[z]; b0 = beg[z]; }
    const int r = rp[b0 + j];
    ex[w][e] = (uint32_t)np[b0 + j];
    eb[w][e] = (uint16_t)((2u << q) << 8 | (uint32_t)(r < 0 ? 0 : (r > 255 ? 255 : r)));
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const uint32_t o = eoff[a];
  // unique entries (the first occurrence of each x) with their folded bits and rank, counted per bucket
  // (0: x == aid, 1 + r: rank r <= 31); the others marked 0xFFFF
  for (uint32_t e0 = 0; e0 < tot; e0 += 64) {
    const uint32_t e = e0 + l;
    if (e < tot) {
      const uint32_t x = ex[w][e];
      bool first = true;
      uint32_t bits = 0, rk = 255;
      for (uint32_t f = 0; f < tot; ++f) {
        if (ex[w][f] != x) continue;
        if (f < e) { first = false; break; }
        bits |= eb[w][f] >> 8;
        rk = min(rk, (uint32_t)(eb[w][f] & 0xFFu));
      }
      const int key = x == (uint32_t)a ? 0 : (rk < (uint32_t)ML_TH ? 1 + (int)rk : -1);
      uk[w][e] = first && key >= 0 ? (uint16_t)(bits << 8 | rk) : (uint16_t)0xFFFFu;
      if (first && key >= 0) atomicAdd(&hs[w][key], 1u);
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const uint32_t c = l <= ML_TH ? hs[w][l] : 0u;
  const uint32_t incl = wave_incl_scan(c);
  if (l >= 1 && l <= ML_TH) pc[a * ML_TH + l - 1] = (uint16_t)incl;  // entries of the self bucket and ranks <= l - 1
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  if (l <= ML_TH) hs[w][l] = incl - c;  // bucket starts
  if (l == ML_TH) ucnt[a] = incl;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  for (uint32_t e0 = 0; e0 < tot; e0 += 64) {
    const uint32_t e = e0 + l;
    const uint16_t v = e < tot ? uk[w][e] : (uint16_t)0xFFFFu;
    if (v != 0xFFFFu) {
      const uint32_t x = ex[w][e];
      const int key = x == (uint32_t)a ? 0 : 1 + (int)(v & 0xFFu);
      const uint32_t p = atomicAdd(&hs[w][key], 1u);  // order within a bucket: any (the folds commute)
      mx[o + p] = (int32_t)x;
      mbr[o + p] = v;
    }
  }
}

static __global__ void k_ml_total(CandLists L, uint32_t* __restrict__ tot) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= L.n_items) return;
  uint32_t t = 0;
#pragma unroll
  for (int q = 0; q < CS_SRC; ++q)
    if (L.off[q]) t += L.off[q][a + 1] - L.off[q][a];
  tot[a] = t;
}

struct MergedLists {
  const uint32_t* eoff;   // [n_items] element offset of the aid
  const uint32_t* ucnt;   // [n_items] entries kept in the list (self entry, ranks <= 31)
  const uint16_t* pc;     // [n_items][32] entries a kept aid with trim threshold th takes
  const int32_t* mx;
  const uint16_t* mbr;    // source bits << 8 | min rank
  int32_t n_items;
  const uint32_t* pop_off;
  const int32_t* pop_aid;
  int32_t n_clusters;
};

__device__ __forceinline__ uint32_t cs_hash(uint32_t x, uint32_t mask) { return (x * 0x9E3779B1u >> 9) & mask; }

static __global__ void k_u64_to_u32(const uint64_t* __restrict__ a, int64_t n, uint32_t* __restrict__ b) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = (uint32_t)a[i];
}

// the list pointers of the C-ABI struct, checked (T = ottohip_cand_lists)
template <class T>
static inline int cand_lists_from_abi(const T* lists, CandLists* L, const char* who) {
  for (int q = 0; q < CS_SRC; ++q) {
    L->off[q] = lists->off[q]; L->nxt[q] = lists->nxt[q]; L->rank[q] = lists->rank[q];
    if (L->off[q] && (!L->nxt[q] || !L->rank[q])) { set_error("%s: list %d incomplete", who, q); return OTTOHIP_EINVAL; }
  }
  L->n_items = lists->n_items;
  L->pop_off = lists->pop_off; L->pop_aid = lists->pop_aid; L->n_clusters = lists->pop_off ? lists->n_clusters : 0;
  return 0;
}

// per-aid merged source lists in the context's workspace (once per call); err: the caller's device flag word
// (bit 4: an aid with more than ML_MAX list entries)
static inline int build_merged_lists(Ctx* ctx, const CandLists& L, MergedLists* Mo, int* err, hipStream_t s,
                                     const char* who) {
  Workspace& ws = ctx->ws;
  MergedLists& M = *Mo;
  M.n_items = L.n_items;
  M.pop_off = L.pop_off; M.pop_aid = L.pop_aid; M.n_clusters = L.n_clusters;
  int rc;
  uint32_t *tot_e, *ucnt, *eoff32;
  uint16_t* pc;
  uint64_t *eoff, *etot;
  int32_t* mx;
  uint16_t* mbr;
  const int64_t NI = std::max<int32_t>(L.n_items, 1);
  if ((rc = ws.get("ml_tot", (size_t)NI + 1, &tot_e)) || (rc = ws.get("ml_eoff", (size_t)NI + 1, &eoff)) ||
      (rc = ws.get("ml_eoff32", (size_t)NI + 1, &eoff32)) || (rc = ws.get("ml_ucnt", (size_t)NI, &ucnt)) ||
      (rc = ws.get("ml_etot", 1, &etot)) || (rc = ws.get("ml_pc", (size_t)NI * ML_TH, &pc)))
    return rc;
  int ph0 = ctx->begin("cand_merge_lists", s, 0);
  hipMemsetAsync(tot_e + NI, 0, 4, s);
  k_ml_total<<<grid_for(NI), 256, 0, s>>>(L, tot_e);
  if ((rc = exclusive_scan_u32(ctx, tot_e, eoff, NI + 1, etot, s))) return rc;
  uint64_t ne = 0;
  if ((rc = d2h(&ne, etot, 1, s))) return rc;
  if (ne >= ((uint64_t)1 << 32)) { set_error("%s: > 2^32 list entries", who); return OTTOHIP_ELIMIT; }
  if ((rc = ws.get("ml_x", (size_t)std::max<uint64_t>(ne, 1), &mx)) ||
      (rc = ws.get("ml_br", (size_t)std::max<uint64_t>(ne, 1), &mbr)))
    return rc;
  k_u64_to_u32<<<grid_for(NI + 1), 256, 0, s>>>(eoff, NI + 1, eoff32);
  k_ml_build<<<(unsigned)ceil_div(NI, 4), 256, 0, s>>>(L, eoff32, mx, mbr, ucnt, pc, err);
  ctx->end(ph0, s);
  M.eoff = eoff32; M.ucnt = ucnt; M.pc = pc; M.mx = mx; M.mbr = mbr;
  return 0;
}

// the candidate handle (C-ABI opaque type)
}  // namespace ottohip

struct ottohip_candidates {
  int64_t n_sessions = 0, n_cand = 0;
  uint64_t* off = nullptr;  // [S + 1]
  int32_t* next = nullptr;
  int16_t* ord = nullptr;
  uint16_t* flags = nullptr;
  void release() {
    ottohip::dev_free(off);
    ottohip::dev_free(next);
    ottohip::dev_free(ord);
    ottohip::dev_free(flags);
    off = nullptr; next = nullptr; ord = nullptr; flags = nullptr;
  }
};
