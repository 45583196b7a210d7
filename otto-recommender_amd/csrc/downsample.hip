// Negative downsampling (model/downsample_retrieved.py), the row gather behind it, and the submission metric
// (model/eval_submission.py) on gfx950. Plain HIP: no inline assembly in this unit.
//
//   draw         h(row) = mix(mix(seed) ^ (uint32(session) << 32 | uint32(aid_next))), mix = splitmix64's finaliser
//                with its increment. mix is a bijection of uint64, so within a frame whose (session, aid_next) pairs
//                are unique all h differ, and "(h, aid_next) smaller" is "h smaller": the kernels compare h.
//                random(row) = negatives of the row's session and target with h smaller; kept iff random < max_n_neg.
//   k_ds_count   one wave per session: n_pos of the three targets and the kept count n_pos + min(n_neg,
//                ceil(max_n_neg)) (0 without a positive), which needs no draw. The counts are scanned into out_off.
//   k_ds_select  one workgroup per session, the three targets in one pass (h is shared). A target whose negatives
//                all survive (n_neg <= ceil(max_n_neg)) or that has no positive needs no rank. Otherwise the session's
//                h and negative bits sit in LDS (DS_LDS_ROWS rows at most) and each lane counts, for its row, the
//                negatives with a smaller h: the other rows' words are broadcast reads. A session above DS_LDS_ROWS
//                takes the same loop over global memory, recomputing h (quadratic in hashes; the reference's sessions
//                end at 2,500 candidates). Output positions: positives in frame order, then kept negatives in frame
//                order, by ballot prefix within a wave and wave totals through LDS.
//   k_gather_rows  a lane owns an output row and a block a group of DS_GCOLS columns: the row index is read once,
//                eight gathered loads are in flight, the stores are coalesced. One launch for all columns.
//   k_sub_recall one wave per session and type: the submitted list (<= 64) one entry per lane, one ballot per label.
#include "prims.h"
#include "table.h"

#include <cmath>

namespace ottohip {

constexpr int DS_T = 256, DS_WAVES = DS_T / 64;
constexpr int DS_LDS_ROWS = 4096;  // the select's path switch: sessions above it rank over global memory
constexpr int DS_MAX_COLS = 128;   // columns of one gather call
constexpr int DS_GCOLS = 16;       // columns per block of the gather
constexpr int SUB_MAX = 64;        // submitted entries per (session, type): the rank stage's keep_top_k bound
// sessions of one call: a launch's work-items stay below 2^32 (one 256-thread workgroup per session in the select)
constexpr int64_t DS_MAX_SESSIONS = (int64_t)1 << 24;

__host__ __device__ __forceinline__ uint64_t ds_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// seed_mix = ds_mix(seed)
__host__ __device__ __forceinline__ uint64_t ds_hash(uint64_t seed_mix, int32_t session, int32_t aid_next) {
  return ds_mix(seed_mix ^ (((uint64_t)(uint32_t)session << 32) | (uint64_t)(uint32_t)aid_next));
}
// negatives kept of a session with n_pos > 0 positives and n_neg negatives: the rows with random < max_n_neg,
// max_n_neg = min(n_pos * ratio, cap) in float64, random a permutation of [0, n_neg)
__device__ __forceinline__ int64_t ds_keep_neg(int64_t n_pos, int64_t n_neg, double ratio, double cap) {
  const double m = fmin((double)n_pos * ratio, cap);
  return m >= (double)n_neg ? n_neg : (int64_t)ceil(m);
}

struct DsTargets {
  const int8_t* tgt[3];   // NULL: the target is not asked for
  uint32_t* n_pos[3];     // [S]
  uint32_t* cnt[3];       // [S + 1], cnt[S] = 0
  const uint64_t* off[3]; // [S + 1]
  int64_t* rows[3];
};

__device__ __forceinline__ void ds_session(const int64_t* cand_off, int64_t s, int64_t n_rows, int64_t& a, int64_t& b) {
  const int64_t o = cand_off[0];
  a = min(max(cand_off[s] - o, (int64_t)0), n_rows);
  b = min(max(cand_off[s + 1] - o, a), n_rows);
}

__global__ __launch_bounds__(DS_T) void k_ds_count(const int64_t* __restrict__ cand_off, int64_t S, int64_t n_rows,
                                                   const DsTargets T, double ratio, double cap) {
  const int64_t s = (int64_t)blockIdx.x * DS_WAVES + (threadIdx.x >> 6);
  if (s > S) return;  // wave-uniform
  const uint32_t l = lane_id();
  if (s == S) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (l == 0u && T.tgt[t]) T.cnt[t][S] = 0u;
    return;
  }
  int64_t a, b;
  ds_session(cand_off, s, n_rows, a, b);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (!T.tgt[t]) continue;
    uint64_t np = 0;
    for (int64_t i = a + l; i < b; i += 64) np += T.tgt[t][i] != 0;
    np = wave_sum64(np);
    if (l == 0u) {
      const int64_t n_neg = (b - a) - (int64_t)np;
      T.n_pos[t][s] = (uint32_t)np;
      T.cnt[t][s] = np ? (uint32_t)((int64_t)np + ds_keep_neg((int64_t)np, n_neg, ratio, cap)) : 0u;
    }
  }
}

// the session's rows as the rank loop reads them: h and the bits of the targets the row is a ranked negative of
struct DsLdsRows {
  const uint64_t* h;
  const uint8_t* neg;
  __device__ __forceinline__ uint64_t hash(int64_t j) const { return h[j]; }
  __device__ __forceinline__ uint32_t bits(int64_t j) const { return neg[j]; }
};
struct DsGlobalRows {
  const int32_t* session;
  const int32_t* aid_next;
  const int8_t* tgt[3];
  int64_t a;
  uint64_t seed_mix;
  uint32_t rmask;
  __device__ __forceinline__ uint64_t hash(int64_t j) const { return ds_hash(seed_mix, session[a + j], aid_next[a + j]); }
  __device__ __forceinline__ uint32_t bits(int64_t j) const {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if ((rmask >> t) & 1u) m |= (tgt[t][a + j] == 0 ? 1u : 0u) << t;
    return m;
  }
};

// the rows [0, n) of one session: every lane ranks its rows and the block writes the targets' row lists
template <class R>
__device__ __forceinline__ void ds_emit(const R& rows, int64_t a, int64_t n, const DsTargets& T, int64_t s,
                                        const int64_t* npos, const int64_t* keep, uint32_t amask, uint32_t rmask,
                                        uint32_t (*wcnt)[DS_WAVES]) {
  const uint32_t l = lane_id(), w = threadIdx.x >> 6;
  int64_t base[6] = {0, 0, 0, 0, 0, 0};  // written so far: positives of t at [t], kept negatives at [3 + t]
  for (int64_t c = 0; c < n; c += DS_T) {
    const int64_t i = c + threadIdx.x;
    const bool live = i < n;
    uint32_t r0 = 0, r1 = 0, r2 = 0;
    if (rmask) {  // block-uniform
      const uint64_t mine = live ? rows.hash(i) : 0ull;
      // equal h means an equal (session, aid_next), which a valid frame does not hold; the earlier row then goes
      // first, so the ranks stay a permutation and the kept count stays the one k_ds_count reserved
      for (int64_t j = 0; j < n; ++j) {
        const uint64_t hj = rows.hash(j);
        const uint32_t m = (hj < mine || (hj == mine && j < i)) ? rows.bits(j) : 0u;
        r0 += m & 1u;
        r1 += (m >> 1) & 1u;
        r2 += (m >> 2) & 1u;
      }
    }
    const uint32_t rk[3] = {r0, r1, r2};
    bool flag[6];
    uint32_t pre[6];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const bool on = live && ((amask >> t) & 1u);
      const bool pos = on && T.tgt[t][a + i] != 0;
      flag[t] = pos;
      flag[3 + t] = on && !pos && (((rmask >> t) & 1u) == 0u || (int64_t)rk[t] < keep[t]);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const uint64_t bal = __ballot(flag[q]);
      pre[q] = mbcnt(bal);
      if (l == 0u) wcnt[q][w] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int v = 0; v < DS_WAVES; ++v) {
        const uint32_t x = wcnt[q][v];
        before += (uint32_t)v < w ? x : 0u;
        total += x;
      }
      const int t = q % 3;
      if (flag[q]) T.rows[t][(int64_t)T.off[t][s] + (q < 3 ? 0 : npos[t]) + base[q] + before + pre[q]] = a + i;
      base[q] += total;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(DS_T) void k_ds_select(const int64_t* __restrict__ cand_off, int64_t S, int64_t n_rows,
                                                    const int32_t* __restrict__ session,
                                                    const int32_t* __restrict__ aid_next, const DsTargets T,
                                                    double ratio, double cap, uint64_t seed_mix) {
  __shared__ uint64_t l_h[DS_LDS_ROWS];
  __shared__ uint8_t l_neg[DS_LDS_ROWS];
  __shared__ uint32_t l_wcnt[6][DS_WAVES];
  const int64_t s = blockIdx.x;
  if (s >= S) return;
  int64_t a, b;
  ds_session(cand_off, s, n_rows, a, b);
  const int64_t n = b - a;
  // block-uniform: the targets with rows to write (amask) and those whose negatives have to be ranked (rmask)
  int64_t npos[3] = {0, 0, 0}, keep[3] = {0, 0, 0};
  uint32_t amask = 0, rmask = 0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    if (!T.tgt[t]) continue;
    npos[t] = (int64_t)T.n_pos[t][s];
    if (npos[t] == 0) continue;
    amask |= 1u << t;
    keep[t] = ds_keep_neg(npos[t], n - npos[t], ratio, cap);
    if (keep[t] < n - npos[t]) rmask |= 1u << t;
  }
  if (n == 0 || amask == 0u) return;
  if (n <= DS_LDS_ROWS) {
    if (rmask) {
      for (int64_t i = threadIdx.x; i < n; i += DS_T) {
        l_h[i] = ds_hash(seed_mix, session[a + i], aid_next[a + i]);
        uint32_t m = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t)
          if ((rmask >> t) & 1u) m |= (T.tgt[t][a + i] == 0 ? 1u : 0u) << t;
        l_neg[i] = (uint8_t)m;
      }
      __syncthreads();
    }
    ds_emit(DsLdsRows{l_h, l_neg}, a, n, T, s, npos, keep, amask, rmask, l_wcnt);
  } else {
    const DsGlobalRows R{session, aid_next, {T.tgt[0], T.tgt[1], T.tgt[2]}, a, seed_mix, rmask};
    ds_emit(R, a, n, T, s, npos, keep, amask, rmask, l_wcnt);
  }
}

// ---------------------------------------------------------------- gather
struct GatherCols {
  const void* src[DS_MAX_COLS];
  void* dst[DS_MAX_COLS];
  uint8_t dt[DS_MAX_COLS];  // 0 int8, 1 int16, 2 int32, 3 float32 (moved as 32-bit words)
};

__device__ __forceinline__ uint32_t ds_load(const void* p, uint32_t dt, int64_t r) {
  if (dt == 0u) return reinterpret_cast<const uint8_t*>(p)[r];
  if (dt == 1u) return reinterpret_cast<const uint16_t*>(p)[r];
  return reinterpret_cast<const uint32_t*>(p)[r];
}
__device__ __forceinline__ void ds_store(void* p, uint32_t dt, int64_t o, uint32_t v) {
  if (dt == 0u) reinterpret_cast<uint8_t*>(p)[o] = (uint8_t)v;
  else if (dt == 1u) reinterpret_cast<uint16_t*>(p)[o] = (uint16_t)v;
  else reinterpret_cast<uint32_t*>(p)[o] = v;
}

__global__ __launch_bounds__(DS_T) void k_gather_rows(const GatherCols C, int n_cols, const int64_t* __restrict__ rows,
                                                      int64_t n_out, int64_t n_src, int* __restrict__ err) {
  const int c0 = (int)blockIdx.y * DS_GCOLS, c1 = min(c0 + DS_GCOLS, n_cols);
  for (int64_t o = (int64_t)blockIdx.x * DS_T + threadIdx.x; o < n_out; o += (int64_t)gridDim.x * DS_T) {
    int64_t r = rows[o];
    if (r < 0 || r >= n_src) {  // reported by the host; the row reads index 0 and is not a valid output
      if (c0 == 0) atomicOr(err, 1);
      r = 0;
    }
    for (int c = c0; c < c1; c += 8) {
      uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c + j < c1) v[j] = ds_load(C.src[c + j], C.dt[c + j], r);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c + j < c1) ds_store(C.dst[c + j], C.dt[c + j], o, v[j]);
    }
  }
}

// ---------------------------------------------------------------- submission recall
// sums: 256 stripes of [3][2] = {hit, true}
__global__ __launch_bounds__(DS_T) void k_sub_recall(int64_t S, const int64_t* __restrict__ lab_off,
                                                     const int32_t* __restrict__ lab_aid,
                                                     const int64_t* __restrict__ sub_off,
                                                     const int32_t* __restrict__ sub_aid,
                                                     unsigned long long* __restrict__ sums, int* __restrict__ err) {
  const int64_t g = (int64_t)blockIdx.x * DS_WAVES + (threadIdx.x >> 6);
  if (g >= 3 * S) return;  // wave-uniform
  const int64_t t = g / S, s = g - t * S;
  const uint32_t l = lane_id();
  const int64_t lb = lab_off[t * (S + 1) + s], le = lab_off[t * (S + 1) + s + 1];
  const int64_t sb = sub_off[t * (S + 1) + s], se = sub_off[t * (S + 1) + s + 1];
  if (se - sb > SUB_MAX) {
    if (l == 0u) atomicOr(err, 1);
    return;
  }
  if (le <= lb) return;  // submitted rows without labels add nothing
  const bool has = sb + (int64_t)l < se;
  const int32_t mine = has ? sub_aid[sb + l] : 0;
  uint64_t hit = 0, tru = 0;
  for (int64_t j = lb; j < le; ++j) {
    const int32_t y = lab_aid[j];
    const uint32_t m = (uint32_t)__popcll(__ballot(has && mine == y));
    hit += m;
    tru += m > 1u ? m : 1u;
  }
  if (l == 0u) {
    unsigned long long* o = sums + (size_t)(s & 255) * 8 + t * 2;
    atomicAdd(&o[0], (unsigned long long)hit);
    atomicAdd(&o[1], (unsigned long long)(tru < 20u ? tru : 20u));
  }
}

}  // namespace ottohip

using namespace ottohip;

extern "C" {

uint64_t ottohip_downsample_hash(uint64_t seed, int32_t session, int32_t aid_next) {
  return ds_hash(ds_mix(seed), session, aid_next);
}

int ottohip_downsample_lds_rows(void) { return DS_LDS_ROWS; }

int ottohip_downsample_plan(ottohip_ctx* ctx, const int64_t* cand_off, int64_t n_sessions, int64_t n_rows,
                            const int32_t* session, const int32_t* aid_next, const int8_t* const* targets,
                            double keep_ratio_neg_to_pos, double max_neg_per_session, uint64_t seed,
                            int64_t* const* out_off, int64_t* const* out_rows, int64_t out_cap, int64_t* n_out,
                            void* stream) {
  if (!ctx || !cand_off || !targets || !out_off || !n_out || n_sessions < 0 || n_rows < 0 || out_cap < 0 ||
      !(keep_ratio_neg_to_pos >= 0.0) || !(max_neg_per_session >= 0.0)) {
    set_error("downsample_plan: bad arguments (cand_off, targets, out_off, n_out not NULL; ratio and cap >= 0, not NaN)");
    return OTTOHIP_EINVAL;
  }
  bool any = false;
  for (int t = 0; t < 3; ++t) {
    n_out[t] = 0;
    if (!targets[t]) continue;
    any = true;
    if (!out_off[t] || (out_rows && out_cap > 0 && !out_rows[t])) {
      set_error("downsample_plan: target %d has no out_off or out_rows", t); return OTTOHIP_EINVAL;
    }
  }
  if (n_rows > 0 && any && (!session || !aid_next)) {
    set_error("downsample_plan: session and aid_next are needed"); return OTTOHIP_EINVAL;
  }
  if (!any) return 0;
  if (n_sessions >= DS_MAX_SESSIONS) {
    set_error("downsample_plan: %lld sessions, a call takes fewer than 2^24: pass the frame in session ranges",
              (long long)n_sessions);
    return OTTOHIP_ELIMIT;
  }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const int64_t S1 = n_sessions + 1;
  uint32_t* scratch = nullptr;
  OH_TRY(ctx->ws.get("ds_counts", (size_t)S1 * 6, &scratch));
  DsTargets T;
  for (int t = 0; t < 3; ++t) {
    T.tgt[t] = targets[t];
    T.n_pos[t] = scratch + (size_t)t * 2 * S1;
    T.cnt[t] = scratch + (size_t)(t * 2 + 1) * S1;
    T.off[t] = reinterpret_cast<const uint64_t*>(out_off[t]);
    T.rows[t] = out_rows ? out_rows[t] : nullptr;
  }
  ctx->reset_timing();
  int ph = ctx->begin("downsample_count", s, (double)n_rows * 3.0);
  k_ds_count<<<(unsigned)ceil_div(S1, DS_WAVES), DS_T, 0, s>>>(cand_off, n_sessions, n_rows, T, keep_ratio_neg_to_pos,
                                                               max_neg_per_session);
  for (int t = 0; t < 3; ++t)
    if (targets[t])
      OH_TRY(exclusive_scan_u32(ctx, T.cnt[t], reinterpret_cast<uint64_t*>(out_off[t]), S1, nullptr, s));
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  for (int t = 0; t < 3; ++t) {
    if (!targets[t]) continue;
    uint64_t h = 0;
    OH_TRY(d2h(&h, reinterpret_cast<const uint64_t*>(out_off[t]) + n_sessions, 1, s));
    n_out[t] = (int64_t)h;
  }
  if (!out_rows) return 0;
  for (int t = 0; t < 3; ++t)
    if (n_out[t] > out_cap) {
      set_error("downsample_plan: target %d keeps %lld rows, out_cap is %lld", t, (long long)n_out[t], (long long)out_cap);
      return OTTOHIP_EINVAL;
    }
  if (n_sessions == 0 || n_rows == 0) return 0;
  ph = ctx->begin("downsample_select", s, (double)n_rows * 11.0);
  k_ds_select<<<(unsigned)n_sessions, DS_T, 0, s>>>(cand_off, n_sessions, n_rows, session, aid_next, T,
                                                    keep_ratio_neg_to_pos, max_neg_per_session, ds_mix(seed));
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  return 0;
}

int ottohip_gather_rows(ottohip_ctx* ctx, const void* const* src_cols, void* const* dst_cols, const int* col_dtype,
                        int n_cols, const int64_t* rows, int64_t n_out, int64_t n_src_rows, void* stream) {
  if (!ctx || n_cols < 0 || n_cols > DS_MAX_COLS || n_out < 0 || n_src_rows < 0 ||
      (n_cols > 0 && (!src_cols || !dst_cols || !col_dtype)) || (n_out > 0 && !rows)) {
    set_error("gather_rows: bad arguments (0 <= n_cols <= %d)", DS_MAX_COLS); return OTTOHIP_EINVAL;
  }
  GatherCols C;
  memset(&C, 0, sizeof(C));
  for (int c = 0; c < n_cols; ++c) {
    if (col_dtype[c] < 0 || col_dtype[c] > 3 || (n_out > 0 && (!src_cols[c] || !dst_cols[c]))) {
      set_error("gather_rows: column %d: dtype code %d or a NULL pointer", c, col_dtype[c]); return OTTOHIP_EINVAL;
    }
    C.src[c] = src_cols[c];
    C.dst[c] = dst_cols[c];
    C.dt[c] = (uint8_t)col_dtype[c];
  }
  if (n_out == 0 || n_cols == 0) return 0;
  if (n_src_rows == 0) { set_error("gather_rows: rows asked of an empty frame"); return OTTOHIP_ERANGE; }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  int* err = nullptr;
  OH_TRY(ctx->ws.get("ds_err", 1, &err));
  OH_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
  ctx->reset_timing();
  double bytes = 0;
  for (int c = 0; c < n_cols; ++c) bytes += C.dt[c] == 0 ? 1 : (C.dt[c] == 1 ? 2 : 4);
  const int ph = ctx->begin("gather_rows", s, (double)n_out * (2.0 * bytes + 8.0 * (double)ceil_div(n_cols, DS_GCOLS)));
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n_out, DS_T), (int64_t)ctx->n_cu * 8),
                  (unsigned)ceil_div(n_cols, DS_GCOLS));
  k_gather_rows<<<grid, DS_T, 0, s>>>(C, n_cols, rows, n_out, n_src_rows, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) { set_error("gather_rows: a row index is outside [0, %lld)", (long long)n_src_rows); return OTTOHIP_ERANGE; }
  return 0;
}

int ottohip_submission_recall(ottohip_ctx* ctx, int64_t n_sessions, const int64_t* lab_off, const int32_t* lab_aid,
                              const int64_t* sub_off, const int32_t* sub_aid, int64_t* sums_out, void* stream) {
  if (!ctx || !sums_out || n_sessions < 0 || (n_sessions > 0 && (!lab_off || !sub_off))) {
    set_error("submission_recall: bad arguments"); return OTTOHIP_EINVAL;
  }
  for (int i = 0; i < 6; ++i) sums_out[i] = 0;
  if (n_sessions == 0) return 0;
  if (n_sessions >= DS_MAX_SESSIONS) {
    set_error("submission_recall: %lld sessions, a call takes fewer than 2^24 (the sums are additive over session sets)",
              (long long)n_sessions);
    return OTTOHIP_ELIMIT;
  }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  unsigned long long* sums = nullptr;
  int* err = nullptr;
  OH_TRY(ctx->ws.get("sub_sums", 256 * 8, &sums));
  OH_TRY(ctx->ws.get("ds_err", 1, &err));
  OH_HIP(hipMemsetAsync(sums, 0, 256 * 8 * 8, s));
  OH_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
  ctx->reset_timing();
  const int ph = ctx->begin("submission_recall", s, 0);
  k_sub_recall<<<(unsigned)ceil_div(3 * n_sessions, DS_WAVES), DS_T, 0, s>>>(n_sessions, lab_off, lab_aid, sub_off,
                                                                             sub_aid, sums, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  std::vector<unsigned long long> h(256 * 8);
  OH_TRY(d2h(h.data(), sums, h.size(), s));
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) {
    set_error("submission_recall: a (session, type) has more than %d submitted entries", SUB_MAX); return OTTOHIP_EINVAL;
  }
  for (int k = 0; k < 256; ++k)
    for (int i = 0; i < 6; ++i) sums_out[i] += (int64_t)h[(size_t)k * 8 + i];
  return 0;
}

}  // extern "C"
