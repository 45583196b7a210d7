// Rank stage (model/rank.py): LightGBM booster scoring and the per-session top-k on gfx950.
//
//   lowering   every split compares in its column's own type. Integer columns: v <= t <=> v <= floor(t). Float32
//              columns: the staged value is the order-preserving int32 key of its bits, the threshold the key of the
//              largest float32 not above t (a zero of either sign -> key 0, so -0.0 <= 0.0 holds). NaN stages as
//              RK_NAN (INT32_MIN), and each node carries where that key goes: the NaN rule of its missing type on a
//              float column, the plain compare of the value INT32_MIN on an integer column. A missing == zero node
//              carries a flag, and the band |v| <= 1e-35f is the key range [RK_ZLO, RK_ZHI] (floats) or [0, 0] (ints).
//   layout     a forest is one array of 8-byte slots. A slot is an internal node {threshold key, packed word} or a
//              leaf's float64 value; the two children of a node are adjacent (child, child + 1) and the node's word
//              says which of them are leaves. Slot 0 is a dummy node read by finished lanes, slot 1 the +0.0 that
//              pads the tree count to the traversal's interleave.
//   k_rank_score  a lane owns a row. Each wave stages its 64 rows of the used columns in LDS as keys (the lane reads
//              back only its own words: no barrier, no bank conflict); the block's forest sits beside the tiles when
//              it fits, else the slots are read from global memory. Fixed-trip traversal of the forest's depth, eight
//              trees in flight per lane; the leaf values are added in tree order in float64 (no fast-math flag).
//   k_rank_topk   one wave per (session, forest): 64 candidates at a time are sorted by (score desc, position asc)
//              and merged into the running best 64 (the shape of knn.hip's best list, with a 96-bit key).
#include "prims.h"
#include "table.h"

#include <cmath>
#include <limits>

namespace ottohip {

constexpr int RK_MAX_COLS = 128;        // used columns of a ranker (7 bits of a node word)
constexpr int RK_MAX_SLOTS = 1 << 19;   // slots of one forest (19 bits of a node word)
#ifndef OH_RK_IL
#define OH_RK_IL 8  // trees in flight per lane (A/B build flag)
#endif
constexpr int RK_T = 256, RK_WAVES = RK_T / 64, RK_IL = OH_RK_IL;
constexpr size_t RK_LDS = 160 * 1024;   // LDS of a gfx950 CU
constexpr int RK_KMAX = 64;
constexpr int32_t RK_NAN = std::numeric_limits<int32_t>::min();
constexpr int32_t RK_ZHI = (int32_t)__builtin_bit_cast(uint32_t, 1e-35f);  // key of +1e-35f (kZeroThreshold)
constexpr int32_t RK_ZLO = ~RK_ZHI;                                        // key of -1e-35f
constexpr uint32_t RK_DONE = 0x80000000u;
// node word: column slot [0,7) | flags [7,13) | child [13,32)
constexpr uint32_t RK_NANL = 1u << 7, RK_ZB = 1u << 8, RK_ZL = 1u << 9, RK_ISF = 1u << 10, RK_LL = 1u << 11,
                   RK_RL = 1u << 12;
constexpr int RK_CHILD_SHIFT = 13;

__host__ __device__ __forceinline__ int32_t rk_float_key(uint32_t b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) return RK_NAN;
  return (int32_t)(b ^ ((uint32_t)((int32_t)b >> 31) & 0x7fffffffu));
}

struct RankCols {  // the used columns grouped by dtype code: slots [first[d], first[d + 1]) have dtype d
  const void* p[RK_MAX_COLS];
  int32_t first[5];
};
struct RankForest {
  uint32_t slot_off, n_slots, root_off, n_roots;  // n_roots: trees padded to RK_IL
  int32_t depth, in_lds;
  int32_t has_band, pad_;  // a node with missing == zero
};

// the lane's key of a column slot: its word of the staged tile
struct RankKeys {
  const int32_t* tile;  // the lane's word of column slot 0
  __device__ __forceinline__ int32_t operator()(uint32_t slot) const { return tile[slot * 64u]; }
};

// one level of one tree for this lane
template <bool BAND, class P>
__device__ __forceinline__ uint32_t rk_step(uint32_t n, P nodes, const RankKeys& tile) {
  const uint32_t idx = (int32_t)n < 0 ? 0u : n;
  const uint2 nd = nodes[idx];
  const uint32_t w = nd.y;
  const int32_t key = tile(w & 127u);
  bool left = key <= (int32_t)nd.x;
  if constexpr (BAND) {
    const int32_t blo = (w & RK_ISF) ? RK_ZLO : 0, bhi = (w & RK_ISF) ? RK_ZHI : 0;
    if ((w & RK_ZB) && key >= blo && key <= bhi) left = (w & RK_ZL) != 0u;
  }
  if (key == RK_NAN) left = (w & RK_NANL) != 0u;
  const uint32_t leaf = (w & (left ? RK_LL : RK_RL)) ? RK_DONE : 0u;
  const uint32_t nn = ((w >> RK_CHILD_SHIFT) + (left ? 0u : 1u)) | leaf;
  return (int32_t)n < 0 ? n : nn;
}

template <bool BAND, class P, class R>
__device__ __forceinline__ double rk_score(P nodes, R roots, int n_roots, int depth, const RankKeys& tile) {
  double acc = 0.0;
  for (int t = 0; t < n_roots; t += RK_IL) {
    uint32_t n[RK_IL];
#pragma unroll
    for (int j = 0; j < RK_IL; ++j) n[j] = roots[t + j];
    for (int d = 0; d < depth; ++d) {
#pragma unroll
      for (int j = 0; j < RK_IL; ++j) n[j] = rk_step<BAND>(n[j], nodes, tile);
    }
#pragma unroll
    for (int j = 0; j < RK_IL; ++j) {
      const uint2 v = nodes[n[j] & ~RK_DONE];
      acc += __hiloint2double((int)v.y, (int)v.x);
    }
  }
  return acc;
}

// the lane's row of the column slots [c0, c1), all of element type T, into its tile words: eight loads in flight
template <class T, bool FLOAT>
__device__ __forceinline__ void rk_stage(const RankCols& C, int c0, int c1, int64_t row, int32_t* tile) {
  int c = c0;
  for (; c + 8 <= c1; c += 8) {
    T v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = reinterpret_cast<const T*>(C.p[c + j])[row];
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[(c + j) * 64] = FLOAT ? rk_float_key((uint32_t)v[j]) : (int32_t)v[j];
  }
  for (; c < c1; ++c) {
    const T v = reinterpret_cast<const T*>(C.p[c])[row];
    tile[c * 64] = FLOAT ? rk_float_key((uint32_t)v) : (int32_t)v;
  }
}

// dynamic LDS: [forest slots: f_slots x 8 B][forest roots: f_roots x 4 B][RK_WAVES tiles of n_used x 64 words]
__global__ __launch_bounds__(RK_T) void k_rank_score(const RankCols C, int n_used, const RankForest* __restrict__ fd,
                                                     int n_forests, const uint2* __restrict__ slots,
                                                     const uint32_t* __restrict__ roots, int f_slots, int f_roots,
                                                     int64_t n_rows, double* __restrict__ scores) {
  extern __shared__ uint2 rk_lds[];
  uint2* const l_slots = rk_lds;
  uint32_t* const l_roots = reinterpret_cast<uint32_t*>(rk_lds + f_slots);
  const uint32_t l = lane_id(), w = threadIdx.x >> 6;
  int resident = -1;  // the forest whose slots the LDS holds
  int32_t* const tile = reinterpret_cast<int32_t*>(l_roots + f_roots) + (size_t)w * (size_t)max(n_used, 1) * 64u + l;
  if (n_used == 0) tile[0] = 0;
  for (int64_t base = (int64_t)blockIdx.x * RK_T; base < n_rows; base += (int64_t)gridDim.x * RK_T) {
    const int64_t row = base + threadIdx.x;
    const bool live = row < n_rows;
    const RankKeys keys{tile};
    const int64_t srow = live ? row : n_rows - 1;  // a dead lane stages a valid row and writes no score
    rk_stage<int8_t, false>(C, C.first[0], C.first[1], srow, tile);
    rk_stage<int16_t, false>(C, C.first[1], C.first[2], srow, tile);
    rk_stage<int32_t, false>(C, C.first[2], C.first[3], srow, tile);
    rk_stage<uint32_t, true>(C, C.first[3], C.first[4], srow, tile);
    for (int f = 0; f < n_forests; ++f) {
      const RankForest F = fd[f];
      double acc;
      if (F.in_lds) {
        if (resident != f) {  // block-uniform
          __syncthreads();
          for (uint32_t i = threadIdx.x; i < F.n_slots; i += RK_T) l_slots[i] = slots[F.slot_off + i];
          for (uint32_t i = threadIdx.x; i < F.n_roots; i += RK_T) l_roots[i] = roots[F.root_off + i];
          __syncthreads();
          resident = f;
        }
        acc = F.has_band ? rk_score<true>(l_slots, l_roots, (int)F.n_roots, F.depth, keys)
                         : rk_score<false>(l_slots, l_roots, (int)F.n_roots, F.depth, keys);
      } else {
        acc = F.has_band ? rk_score<true>(slots + F.slot_off, roots + F.root_off, (int)F.n_roots, F.depth, keys)
                         : rk_score<false>(slots + F.slot_off, roots + F.root_off, (int)F.n_roots, F.depth, keys);
      }
      if (live) scores[(int64_t)f * n_rows + row] = acc;
    }
  }
}

// ---------------------------------------------------------------- top-k
// (K, P) ascending = (score descending, position ascending); the pad (~0, ~0) sorts last
__device__ __forceinline__ bool rk_less(uint64_t ak, uint32_t ap, uint64_t bk, uint32_t bp) {
  return ak < bk || (ak == bk && ap < bp);
}
__device__ __forceinline__ void rk_cx(uint64_t& K, uint32_t& P, uint32_t l, int j, bool take_min) {
  const uint64_t ok = shfl64(K, (int)(l ^ (uint32_t)j));
  const uint32_t op = (uint32_t)__shfl((int)P, (int)(l ^ (uint32_t)j));
  const bool mine = rk_less(K, P, ok, op) == take_min;
  K = mine ? K : ok;
  P = mine ? P : op;
}
__device__ __forceinline__ void rk_sort64(uint64_t& K, uint32_t& P, uint32_t l) {
#pragma unroll
  for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) rk_cx(K, P, l, j, ((l & kk) == 0) == ((l & j) == 0));
  }
}
// the 64 first of two ascending runs: min(best[l], run[63 - l]) is bitonic, one merge sorts it
__device__ __forceinline__ void rk_merge64(uint64_t& bK, uint32_t& bP, uint64_t K, uint32_t P, uint32_t l) {
  const uint64_t rk = shfl64(K, (int)(63u - l));
  const uint32_t rp = (uint32_t)__shfl((int)P, (int)(63u - l));
  if (rk_less(rk, rp, bK, bP)) { bK = rk; bP = rp; }
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) rk_cx(bK, bP, l, j, (l & j) == 0);
}

__device__ __forceinline__ void rk_session(const int64_t* cand_off, int64_t s, int64_t n_rows, int64_t& a, int64_t& b) {
  const int64_t o = cand_off[0];
  a = min(max(cand_off[s] - o, (int64_t)0), n_rows);
  b = min(max(cand_off[s + 1] - o, a), n_rows);
}

__global__ __launch_bounds__(256) void k_rank_kept(const int64_t* __restrict__ cand_off, int64_t S, int64_t n_rows,
                                                   int k, uint32_t* __restrict__ cnt) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s > S) return;
  if (s == S) { cnt[s] = 0u; return; }
  int64_t a, b;
  rk_session(cand_off, s, n_rows, a, b);
  cnt[s] = (uint32_t)min(b - a, (int64_t)k);
}

__global__ __launch_bounds__(256) void k_rank_topk(const double* __restrict__ scores, int n_forests, int64_t n_rows,
                                                   const int64_t* __restrict__ cand_off, int64_t S,
                                                   const int32_t* __restrict__ aid_next, int k,
                                                   const uint64_t* __restrict__ out_off, int64_t out_cap,
                                                   int32_t* __restrict__ out_session, int32_t* __restrict__ out_aid,
                                                   double* __restrict__ out_score, int16_t* __restrict__ out_rank) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= S * n_forests) return;  // wave-uniform
  const int64_t f = g / S, s = g - f * S;
  const uint32_t l = lane_id();
  int64_t a, b;
  rk_session(cand_off, s, n_rows, a, b);
  const double* sc = scores + f * n_rows;
  uint64_t bK = ~0ull;
  uint32_t bP = ~0u;
  for (int64_t c = a; c < b; c += 64) {
    const int64_t i = c + l;
    uint64_t K = ~0ull;
    uint32_t P = ~0u;
    if (i < b) {
      double v = sc[i];
      if (v == 0.0) v = 0.0;  // -0.0 ranks as 0.0
      const uint64_t u = (uint64_t)__double_as_longlong(v);
      K = ~(u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull));
      P = (uint32_t)(i - a);
    }
    // a chunk with nothing ahead of the worst kept entry changes nothing
    const uint64_t wK = shfl64(bK, 63);
    const uint32_t wP = (uint32_t)__shfl((int)bP, 63);
    if (__ballot(rk_less(K, P, wK, wP)) == 0ull) continue;
    rk_sort64(K, P, l);
    rk_merge64(bK, bP, K, P, l);
  }
  const int64_t kept = min(b - a, (int64_t)k);
  if ((int64_t)l < kept) {
    const int64_t o = f * out_cap + (int64_t)out_off[s] + l;
    out_session[o] = (int32_t)s;
    out_aid[o] = aid_next[a + bP];
    out_score[o] = sc[a + bP];
    out_rank[o] = (int16_t)(l + 1);
  }
}

// ---------------------------------------------------------------- host: lowering and flattening
struct Lowered { int32_t key; uint32_t flags; };

// the split (t, decision_type) on a column of dtype code dt (0 int8, 1 int16, 2 int32, 3 float32)
static int rk_lower(double t, int decision_type, int dt, Lowered* out) {
  const int missing = (decision_type >> 2) & 3;
  if ((decision_type & 1) || missing == 3 || decision_type < 0 || decision_type > 15 || dt < 0 || dt > 3 ||
      !std::isfinite(t))
    return OTTOHIP_EINVAL;
  const bool def_left = (decision_type & 2) != 0;
  uint32_t fl = 0;
  int32_t key;
  if (dt == 3) {
    float f = (float)t;
    if ((double)f > t) f = std::nextafterf(f, -std::numeric_limits<float>::infinity());
    uint32_t b;
    if (f == 0.0f) b = 0u; else memcpy(&b, &f, 4);
    key = rk_float_key(b);
    fl |= RK_ISF;
    // NaN: the default side under missing == NaN; else it is 0.0 (in the zero band under missing == zero)
    const bool nan_left = missing == 2 ? def_left : (missing == 1 ? def_left : 0.0 <= t);
    if (nan_left) fl |= RK_NANL;
  } else {
    const double fl_t = std::floor(t);
    key = fl_t >= 2147483647.0 ? std::numeric_limits<int32_t>::max()
          : (fl_t < -2147483648.0 ? std::numeric_limits<int32_t>::min() : (int32_t)fl_t);
    // the key RK_NAN is the value INT32_MIN here: outside the zero band, so a plain compare
    if (-2147483648.0 <= t) fl |= RK_NANL;
  }
  if (missing == 1) fl |= RK_ZB | (def_left ? RK_ZL : 0u);
  out->key = key;
  out->flags = fl;
  return 0;
}

struct HostForest {
  std::vector<uint64_t> slots;
  std::vector<uint32_t> roots;
  int depth = 0;
  bool has_band = false;
};

static inline uint64_t rk_node(int32_t key, uint32_t word) { return (uint64_t)(uint32_t)key | ((uint64_t)word << 32); }
static inline uint64_t rk_value(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

static int rk_flatten(const ottohip_forest& F, int fi, const int* col_dtype, int n_cols, const std::vector<int>& slot_of,
                      HostForest* out) {
  out->slots.assign(2, 0ull);
  out->slots[0] = rk_node(0, 0u);
  out->slots[1] = rk_value(0.0);
  struct Item { int node; uint32_t slot; int depth; };
  std::vector<Item> q;
  std::vector<char> seen;
  for (int t = 0; t < F.n_trees; ++t) {
    const int64_t o = F.tree_off[t], ni = (int64_t)F.tree_off[t + 1] - o, lo = o + t;
    if (ni < 0) { set_error("ranker_create: forest %d tree %d: tree offsets descend", fi, t); return OTTOHIP_EINVAL; }
    for (int64_t i = 0; i <= ni; ++i)
      if (!std::isfinite(F.leaf_value[lo + i])) {
        set_error("ranker_create: forest %d tree %d: leaf value %lld is not finite", fi, t, (long long)i);
        return OTTOHIP_EINVAL;
      }
    if (ni == 0) {
      out->roots.push_back((uint32_t)out->slots.size() | RK_DONE);
      out->slots.push_back(rk_value(F.leaf_value[lo]));
      continue;
    }
    seen.assign((size_t)ni, 0);
    q.clear();
    out->roots.push_back((uint32_t)out->slots.size());
    q.push_back({0, (uint32_t)out->slots.size(), 0});
    out->slots.push_back(0ull);
    seen[0] = 1;
    for (size_t h = 0; h < q.size(); ++h) {
      const Item it = q[h];
      const int64_t g = o + it.node;
      const int col = F.split_feature[g];
      if (col < 0 || col >= n_cols) {
        set_error("ranker_create: forest %d tree %d: split column %d outside [0, %d)", fi, t, col, n_cols);
        return OTTOHIP_EINVAL;
      }
      Lowered L;
      if (rk_lower(F.threshold[g], F.decision_type[g], col_dtype[col], &L) != 0) {
        set_error("ranker_create: forest %d tree %d node %d: threshold %g / decision_type %d is not a finite numeric split",
                  fi, t, it.node, F.threshold[g], F.decision_type[g]);
        return OTTOHIP_EINVAL;
      }
      if (L.flags & RK_ZB) out->has_band = true;
      const uint32_t child = (uint32_t)out->slots.size();
      if (child + 2u > (uint32_t)RK_MAX_SLOTS) {
        set_error("ranker_create: forest %d has more than %d nodes and leaves", fi, RK_MAX_SLOTS);
        return OTTOHIP_ELIMIT;
      }
      out->slots.push_back(0ull);
      out->slots.push_back(0ull);
      uint32_t word = (uint32_t)slot_of[col] | L.flags | (child << RK_CHILD_SHIFT);
      const int32_t kids[2] = {F.left_child[g], F.right_child[g]};
      for (int side = 0; side < 2; ++side) {
        const int64_t c = kids[side];
        if (c >= 0) {
          if (c >= ni || seen[(size_t)c]) {
            set_error("ranker_create: forest %d tree %d node %d: child %lld is outside the tree or visited twice", fi, t,
                      it.node, (long long)c);
            return OTTOHIP_EINVAL;
          }
          seen[(size_t)c] = 1;
          q.push_back({(int)c, child + (uint32_t)side, it.depth + 1});
        } else {
          const int64_t leaf = ~c;
          if (leaf > ni) {
            set_error("ranker_create: forest %d tree %d node %d: leaf %lld is outside the tree", fi, t, it.node,
                      (long long)leaf);
            return OTTOHIP_EINVAL;
          }
          out->slots[child + side] = rk_value(F.leaf_value[lo + leaf]);
          word |= side == 0 ? RK_LL : RK_RL;
          out->depth = std::max(out->depth, it.depth + 1);
        }
      }
      out->slots[it.slot] = rk_node(L.key, word);
    }
  }
  while (out->roots.size() % RK_IL) out->roots.push_back(1u | RK_DONE);
  return 0;
}

}  // namespace ottohip

using namespace ottohip;

extern "C" {

struct ottohip_ranker {
  int device = 0;
  int n_forests = 0, n_cols = 0, n_used = 0;
  int used_col[RK_MAX_COLS];
  uint8_t used_dt[RK_MAX_COLS];
  RankForest* fd = nullptr;     // device [n_forests]
  uint64_t* slots = nullptr;    // device, all forests
  uint32_t* roots = nullptr;
  int f_slots = 0, f_roots = 0; // LDS forest region (largest resident forest)
  size_t lds = 0;
};

int ottohip_rank_lower(double threshold, int decision_type, int dtype, int32_t* key, int* flags, int32_t* band_lo,
                       int32_t* band_hi) {
  Lowered L;
  if (rk_lower(threshold, decision_type, dtype, &L) != 0) {
    set_error("rank_lower: threshold %g, decision_type %d, dtype %d is not a finite numeric split", threshold,
              decision_type, dtype);
    return OTTOHIP_EINVAL;
  }
  if (key) *key = L.key;
  if (flags) *flags = ((L.flags & RK_NANL) ? 1 : 0) | ((L.flags & RK_ZB) ? 2 : 0) | ((L.flags & RK_ZL) ? 4 : 0);
  if (band_lo) *band_lo = dtype == 3 ? RK_ZLO : 0;
  if (band_hi) *band_hi = dtype == 3 ? RK_ZHI : 0;
  return 0;
}

void ottohip_ranker_free(ottohip_ranker* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();
  if (r->fd) dev_free(r->fd);
  if (r->slots) dev_free(r->slots);
  if (r->roots) dev_free(r->roots);
  delete r;
}

int ottohip_ranker_create(ottohip_ctx* ctx, const ottohip_forest* forests, int n_forests, const int* col_dtype,
                          int n_cols, ottohip_ranker** out) {
  if (!ctx || !forests || !col_dtype || !out || n_forests < 1 || n_forests > 64 || n_cols < 1) {
    set_error("ranker_create: bad arguments (1 <= n_forests <= 64)"); return OTTOHIP_EINVAL;
  }
  for (int c = 0; c < n_cols; ++c)
    if (col_dtype[c] < 0 || col_dtype[c] > 3) { set_error("ranker_create: dtype code of column %d", c); return OTTOHIP_EINVAL; }
  // the columns any split reads, in column order
  std::vector<int> slot_of((size_t)n_cols, -1);
  for (int f = 0; f < n_forests; ++f) {
    const ottohip_forest& F = forests[f];
    if (F.n_trees < 0 || !F.tree_off || !F.leaf_value || F.tree_off[0] != 0) {
      set_error("ranker_create: forest %d: missing arrays", f); return OTTOHIP_EINVAL;
    }
    const int64_t ni = F.tree_off[F.n_trees];
    if (ni > 0 && (!F.split_feature || !F.threshold || !F.decision_type || !F.left_child || !F.right_child)) {
      set_error("ranker_create: forest %d: missing node arrays", f); return OTTOHIP_EINVAL;
    }
    for (int64_t i = 0; i < ni; ++i) {
      const int col = F.split_feature[i];
      if (col < 0 || col >= n_cols) {
        set_error("ranker_create: forest %d: split column %d outside [0, %d)", f, col, n_cols); return OTTOHIP_EINVAL;
      }
      slot_of[(size_t)col] = 0;
    }
  }
  ottohip_ranker* r = new ottohip_ranker();
  r->device = ctx->device;
  r->n_forests = n_forests;
  r->n_cols = n_cols;
  for (int d = 0; d < 4; ++d) {  // slots grouped by dtype code, for the staging loops
    for (int c = 0; c < n_cols; ++c) {
      if (col_dtype[c] != d || slot_of[(size_t)c] < 0) continue;
      if (r->n_used == RK_MAX_COLS) {
        delete r;
        set_error("ranker_create: the forests read more than %d columns", RK_MAX_COLS); return OTTOHIP_ELIMIT;
      }
      slot_of[(size_t)c] = r->n_used;
      r->used_col[r->n_used] = c;
      r->used_dt[r->n_used] = (uint8_t)col_dtype[c];
      ++r->n_used;
    }
  }
  std::vector<uint64_t> slots;
  std::vector<uint32_t> roots;
  std::vector<RankForest> fd((size_t)n_forests);
  const size_t tiles = (size_t)RK_WAVES * (size_t)std::max(r->n_used, 1) * 64u * 4u;
  for (int f = 0; f < n_forests; ++f) {
    HostForest H;
    const int rc = rk_flatten(forests[f], f, col_dtype, n_cols, slot_of, &H);
    if (rc != 0) { delete r; return rc; }
    RankForest& D = fd[(size_t)f];
    D.slot_off = (uint32_t)slots.size();
    D.n_slots = (uint32_t)H.slots.size();
    D.root_off = (uint32_t)roots.size();
    D.n_roots = (uint32_t)H.roots.size();
    D.depth = H.depth;
    D.has_band = H.has_band ? 1 : 0;
    D.pad_ = 0;
    D.in_lds = tiles + H.slots.size() * 8u + H.roots.size() * 4u <= RK_LDS ? 1 : 0;
    if (D.in_lds) {
      r->f_slots = std::max(r->f_slots, (int)H.slots.size());
      r->f_roots = std::max(r->f_roots, (int)H.roots.size());
    }
    slots.insert(slots.end(), H.slots.begin(), H.slots.end());
    roots.insert(roots.end(), H.roots.begin(), H.roots.end());
    if (slots.size() > 0xFFFFFFFFull / 2) { delete r; set_error("ranker_create: forests too large"); return OTTOHIP_ELIMIT; }
  }
  // two resident forests may each fit alone but not the larger slot count beside the larger root count
  while (tiles + (size_t)r->f_slots * 8u + (size_t)r->f_roots * 4u > RK_LDS) {
    int big = -1;
    for (int f = 0; f < n_forests; ++f)
      if (fd[(size_t)f].in_lds && (big < 0 || fd[(size_t)f].n_slots > fd[(size_t)big].n_slots)) big = f;
    fd[(size_t)big].in_lds = 0;
    r->f_slots = r->f_roots = 0;
    for (int f = 0; f < n_forests; ++f)
      if (fd[(size_t)f].in_lds) {
        r->f_slots = std::max(r->f_slots, (int)fd[(size_t)f].n_slots);
        r->f_roots = std::max(r->f_roots, (int)fd[(size_t)f].n_roots);
      }
  }
  if (roots.empty()) roots.assign(RK_IL, 1u | RK_DONE);
  r->lds = tiles + (size_t)r->f_slots * 8u + (size_t)r->f_roots * 4u;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = dev_alloc(reinterpret_cast<void**>(&r->fd), fd.size() * sizeof(RankForest), "rank_forests");
  if (e == hipSuccess) e = dev_alloc(reinterpret_cast<void**>(&r->slots), slots.size() * 8u, "rank_slots");
  if (e == hipSuccess) e = dev_alloc(reinterpret_cast<void**>(&r->roots), roots.size() * 4u, "rank_roots");
  if (e == hipSuccess) e = hipMemcpy(r->fd, fd.data(), fd.size() * sizeof(RankForest), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r->slots, slots.data(), slots.size() * 8u, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r->roots, roots.data(), roots.size() * 4u, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rank_score), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)r->lds);
  if (e != hipSuccess) {
    set_error("ranker_create: %s", hipGetErrorString(e));
    ottohip_ranker_free(r);
    return e == hipErrorOutOfMemory ? OTTOHIP_ENOMEM : OTTOHIP_EHIP;
  }
  *out = r;
  return 0;
}

int ottohip_ranker_info(const ottohip_ranker* r, int* n_forests, int* n_used, int* n_resident, int64_t* lds_bytes) {
  if (!r) { set_error("ranker_info: null ranker"); return OTTOHIP_EINVAL; }
  if (n_forests) *n_forests = r->n_forests;
  if (n_used) *n_used = r->n_used;
  if (lds_bytes) *lds_bytes = (int64_t)r->lds;
  if (n_resident) {
    std::vector<RankForest> fd((size_t)r->n_forests);
    OH_HIP(hipSetDevice(r->device));
    OH_HIP(hipMemcpy(fd.data(), r->fd, fd.size() * sizeof(RankForest), hipMemcpyDeviceToHost));
    *n_resident = 0;
    for (const RankForest& F : fd) *n_resident += F.in_lds;
  }
  return 0;
}

int ottohip_ranker_predict(ottohip_ctx* ctx, const ottohip_ranker* r, void* const* cols, int n_cols, int64_t n_rows,
                           double* scores, void* stream) {
  if (!ctx || !r || !cols || n_cols != r->n_cols || n_rows < 0 || (n_rows > 0 && !scores)) {
    set_error("ranker_predict: bad arguments (n_cols %d, the ranker has %d)", n_cols, r ? r->n_cols : -1);
    return OTTOHIP_EINVAL;
  }
  if (n_rows == 0) return 0;
  RankCols C;
  memset(&C, 0, sizeof(C));
  for (int u = 0; u < r->n_used; ++u) {
    if (!cols[r->used_col[u]]) {
      set_error("ranker_predict: column %d is read by a forest and its pointer is NULL", r->used_col[u]);
      return OTTOHIP_EINVAL;
    }
    C.p[u] = cols[r->used_col[u]];
  }
  for (int d = 0; d <= 4; ++d) {
    C.first[d] = 0;
    for (int u = 0; u < r->n_used; ++u) C.first[d] += r->used_dt[u] < d;
  }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const int64_t tiles = ceil_div(n_rows, RK_T);
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, (int64_t)ctx->n_cu * 4);
  ctx->reset_timing();
  const int ph = ctx->begin("rank_score", s, (double)n_rows * 8.0 * r->n_forests);
  k_rank_score<<<grid, RK_T, r->lds, s>>>(C, r->n_used, r->fd, r->n_forests, reinterpret_cast<const uint2*>(r->slots),
                                          r->roots, r->f_slots, r->f_roots, n_rows, scores);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  return 0;
}

int ottohip_ranker_topk(ottohip_ctx* ctx, const double* scores, int n_forests, int64_t n_rows, const int64_t* cand_off,
                        int64_t n_sessions, const int32_t* aid_next, int k, int64_t out_cap, int64_t* out_off,
                        int32_t* out_session, int32_t* out_aid_next, double* out_score, int16_t* out_rank,
                        void* stream) {
  if (!ctx || n_forests < 1 || n_rows < 0 || n_sessions < 0 || k < 1 || k > RK_KMAX || !cand_off || !out_off ||
      out_cap < 0 || (n_rows > 0 && (!scores || !aid_next)) ||
      (out_cap > 0 && (!out_session || !out_aid_next || !out_score || !out_rank))) {
    set_error("ranker_topk: bad arguments (1 <= k <= %d)", RK_KMAX); return OTTOHIP_EINVAL;
  }
  if (out_cap < std::min<int64_t>(n_rows, n_sessions * k)) {
    set_error("ranker_topk: out_cap %lld is below min(n_rows, n_sessions * k)", (long long)out_cap); return OTTOHIP_EINVAL;
  }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  uint32_t* cnt = nullptr;
  OH_TRY(ctx->ws.get("rank_kept", (size_t)n_sessions + 1, &cnt));
  ctx->reset_timing();
  const int ph = ctx->begin("rank_topk", s, (double)n_rows * 8.0 * n_forests);
  k_rank_kept<<<(unsigned)ceil_div(n_sessions + 1, 256), 256, 0, s>>>(cand_off, n_sessions, n_rows, k, cnt);
  OH_TRY(exclusive_scan_u32(ctx, cnt, reinterpret_cast<uint64_t*>(out_off), n_sessions + 1, nullptr, s));
  if (n_sessions > 0)
    k_rank_topk<<<(unsigned)ceil_div(n_sessions * n_forests, 4), 256, 0, s>>>(
        scores, n_forests, n_rows, cand_off, n_sessions, aid_next, k, reinterpret_cast<const uint64_t*>(out_off), out_cap,
        out_session, out_aid_next, out_score, out_rank);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
