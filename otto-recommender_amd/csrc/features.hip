// Ranker feature columns of retrieve_and_gen_feats (model/retrieve.py:138-232 in full, :293-403,
// :522-602, targets :630-644) for the candidates of a session range of an ottohip_candidates handle.
//
//   k_feat_aids  (R3 in full) one wave per session: the sibling of k_cand_aids that keeps all 20 columns of
//                :208-230 per kept aid (AidRec) and the session statistics of :115-135 (SessRec)
//   k_feat_fold  one wave per session: a lane owns a candidate (tiles of 64) and keeps its accumulators in
//                registers; the wave walks the session's kept aids and, for each, the kept prefix of its merged
//                list (pc[aid][th] entries, plus the self pair) -- both loops wave-uniform; the lane whose
//                aid_next equals the entry takes the pair with the values of every source that lists it (looked
//                up in the source lists by the whole wave). No atomics, no shared accumulators: every
//                aggregate is an integer sum, count, min or max, so any order gives the same bits. Then the
//                lane finalises its candidate (:526-551 means, casts, since_* / rel_pos_*, flags, cl50 / cl1
//                ranks, targets) and writes one value per column.
//
// Semantics (feature columns): aggregates skip nulls and are null (-1 after the final fill) over a
// group without a non-null value, sums included; (aid == aid_next) * col is 0 on a non-self row with a non-null
// col; means are f64(sum) / f64(count), casts truncate, round is half away from zero; integer products in 64 bits.
#include <algorithm>
#include <cstdlib>
#include "prims.h"
#include "table.h"
#include "cand_shared.h"

namespace ottohip {

// (name, dtype code: 0 int8, 1 int16, 2 int32, 3 float32) in the reference's column order
#define FEAT_RULE_COLS(X, R) X(R##_count, 2) X(R##_count_pop, 1) X(R##_perc_pop, 1) X(R##_rank, 1) X(R##_count_rel, 1)
#define FEAT_W2V_COLS(X, W) X(n_w2vec_##W, 1) X(dist_w2vec_##W, 2) X(rank_w2vec_##W, 1) X(best_rank_w2vec_##W, 1)
#define FEAT_COLUMNS(X)                                                                                              \
  X(session, 2) X(aid_next, 2)                                                                                       \
  X(slf_n, 1) X(slf_n_clicks, 1) X(slf_n_carts, 1) X(slf_n_orders, 1)                                                \
  X(slf_rank_by_n, 1) X(slf_rank_by_n_carts, 1) X(slf_rank_by_n_orders, 1)                                           \
  X(slf_ts_rel_pos_in_session, 1) X(slf_ts_order, 1) X(slf_ts_order_rel, 1)                                          \
  X(slf_ts_order_clicks, 1) X(slf_ts_order_carts, 1) X(slf_ts_order_orders, 1) X(slf_left_in_cart, 0)                \
  X(n_uniq_aid, 1) X(n_uniq_aid_clicks, 1) X(n_uniq_aid_carts, 1) X(n_uniq_aid_orders, 1)                            \
  X(n_aid, 1) X(n_aid_clicks, 1) X(n_aid_carts, 1) X(n_aid_orders, 1)                                                \
  X(ts_order_aid, 1) X(ts_order_aid_rel, 1) X(ts_order_aid_clicks, 1) X(ts_order_aid_carts, 1)                       \
  X(ts_order_aid_orders, 1) X(ts_aid_rel_pos_in_session, 1) X(rank_by_n_aid, 1)                                      \
  FEAT_RULE_COLS(X, click_to_click) FEAT_RULE_COLS(X, click_to_cart_or_buy) FEAT_RULE_COLS(X, cart_to_cart)          \
  FEAT_RULE_COLS(X, cart_to_buy) FEAT_RULE_COLS(X, buy_to_buy)                                                       \
  FEAT_W2V_COLS(X, all) FEAT_W2V_COLS(X, 1_2)                                                                        \
  X(n_events_session, 1) X(n_aids_session, 1) X(n_clicks_session, 1) X(n_carts_session, 1) X(n_orders_session, 1)    \
  X(duration_session, 2) X(only_orders_session, 0)                                                                   \
  X(since_ts_aid, 2) X(since_ts_aid_clicks, 2) X(since_ts_aid_carts, 2) X(since_ts_aid_orders, 2)                    \
  X(slf_since_ts, 2) X(slf_since_ts_clicks, 2) X(slf_since_ts_carts, 2) X(slf_since_ts_orders, 2)                    \
  X(since_session_start_ts_aid, 2) X(since_session_start_ts_aid_orders, 2)                                           \
  X(rel_pos_max_ts_aid_in_session, 0) X(rel_pos_mean_max_ts_aid_in_session, 0)                                       \
  X(rel_pos_mean_max_ts_aid_orders_in_session, 0)                                                                    \
  X(src_any, 0) X(src_self, 0) X(src_click_to_click, 0) X(src_click_to_cart_or_buy, 0) X(src_cart_to_cart, 0)        \
  X(src_cart_to_buy, 0) X(src_buy_to_buy, 0) X(src_w2vec_all, 0) X(src_w2vec_1_2, 0)                                 \
  X(rank_clicks_cl50, 1) X(rank_carts_cl50, 1) X(rank_orders_cl50, 1) X(rank_clicks_7d_cl50, 1)                      \
  X(rank_carts_7d_cl50, 1) X(rank_orders_7d_cl50, 1) X(src_pop_cl50, 0)                                              \
  X(rank_clicks_cl1, 1) X(rank_carts_cl1, 1) X(rank_orders_cl1, 1)                                                   \
  X(cos_sim_ses_aid, 3) X(eucl_dist_ses_aid, 3)                                                                      \
  X(target_clicks, 0) X(target_carts, 0) X(target_orders, 0)

#define X(n, d) C_##n,
enum FeatCol : int { FEAT_COLUMNS(X) N_FEAT_COLS };
#undef X
#define X(n, d) #n,
static const char* const kFeatNames[N_FEAT_COLS] = {FEAT_COLUMNS(X)};
#undef X
#define X(n, d) d,
static const int kFeatDtype[N_FEAT_COLS] = {FEAT_COLUMNS(X)};
template <int COL> struct FeatDt {
  static constexpr int all[N_FEAT_COLS] = {FEAT_COLUMNS(X)};
  static constexpr int value = all[COL];
};
#undef X

struct FeatCols { void* p[N_FEAT_COLS]; };
struct FeatVals {
  const int32_t* count[5];
  const int16_t* count_pop[5];
  const int16_t* perc_pop[5];
  const int8_t* count_rel[5];
  const int32_t* dist[2];
  const int16_t* pop_ranks6;
  const int16_t* cl1_ranks3;
};

// all 20 columns of :208-230 for a kept aid; n / mt: [all, clicks, carts, orders], mt < 0 and r_t == 0 are null
struct AidRec {
  int32_t aid, n[4], mt[4], r_ts, r_rel, r_n, r_nc, r_no, r_t[3], rel_pos, lic, th;
};
struct SessRec { int32_t n_events, n_aids, n_type[3], min_ts, max_ts, pad; };

template <int COL>
__device__ __forceinline__ void put(const FeatCols& C, uint64_t i, int32_t v) {
  void* p = C.p[COL];
  if (!p) return;
  constexpr int d = FeatDt<COL>::value;
  if (d == 0) static_cast<int8_t*>(p)[i] = (int8_t)v;
  else if (d == 1) static_cast<int16_t*>(p)[i] = (int16_t)v;
  else static_cast<int32_t*>(p)[i] = v;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// sessions [s_lo, s_lo + n_s): records at rec[off[s] - off[s_lo] + k], k < n_kept[s - s_lo]
__global__ __launch_bounds__(64) void k_feat_aids(const int64_t* __restrict__ off, int64_t s_lo, int64_t n_s,
                                                  const int32_t* __restrict__ aid, const int32_t* __restrict__ ts,
                                                  const int8_t* __restrict__ type, AidRec* __restrict__ rec,
                                                  uint32_t* __restrict__ n_kept, SessRec* __restrict__ srec,
                                                  int* __restrict__ err) {
  __shared__ int32_t ea[CS_MAXE], et[CS_MAXE];
  __shared__ int8_t ey[CS_MAXE];
  __shared__ int32_t ua[CS_MAXE], un[4][CS_MAXE], ut[4][CS_MAXE];  // n / max ts: [all, clicks, carts, orders]
  const int l = threadIdx.x;
  const int64_t si = blockIdx.x;
  if (si >= n_s) return;
  const int64_t s = s_lo + si;
  const int64_t e0 = off[s], eb = off[s_lo];
  const int n = (int)(off[s + 1] - e0);
  if (n > CS_MAXE || n < 0) {
    if (l == 0) { atomicOr(err, 1); n_kept[si] = 0; }
    return;
  }
  int nt[3] = {0, 0, 0}, tmin = INT32_MAX, tmax = INT32_MIN;
  for (int i = l; i < n; i += 64) {
    const int32_t t = ts[e0 + i];
    const int8_t y = type[e0 + i];
    ea[i] = aid[e0 + i]; et[i] = t; ey[i] = y;
    if (t < 0 || y < 0 || y > 2) atomicOr(err, 2);
#pragma unroll
    for (int q = 0; q < 3; ++q) nt[q] += y == q;
    tmin = min(tmin, t); tmax = max(tmax, t);
  }
  __syncthreads();
  // distinct aids (first occurrence), compacted in event order
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + l;
    bool first = i < n;
    if (first) {
      const int32_t a = ea[i];
      for (int j = 0; j < i; ++j)
        if (ea[j] == a) { first = false; break; }
    }
    const uint64_t b = __ballot(first);
    if (first) ua[base + (int)mbcnt(b)] = ea[i];
    base += (int)__popcll(b);
  }
  const int m = base;
  __syncthreads();
  for (int u = l; u < m; u += 64) {
    const int32_t a = ua[u];
    int cnt[4] = {0, 0, 0, 0}, mt[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
    for (int i = 0; i < n; ++i) {
      if (ea[i] != a) continue;
      const int y = ey[i] + 1;
      const int32_t t = et[i];
      cnt[0]++; mt[0] = max(mt[0], t);
#pragma unroll
      for (int q = 1; q < 4; ++q)
        if (q == y) { cnt[q]++; mt[q] = max(mt[q], t); }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { un[q][u] = cnt[q]; ut[q][u] = mt[q]; }
  }
  __syncthreads();
  {
    const int c0 = wave_sum_i32(nt[0]), c1 = wave_sum_i32(nt[1]), c2 = wave_sum_i32(nt[2]);
    const int mn = wave_min_i32(tmin), mx = wave_max_i32(tmax);
    if (l == 0) {
      SessRec r;
      r.n_events = n; r.n_aids = m; r.n_type[0] = c0; r.n_type[1] = c1; r.n_type[2] = c2;
      r.min_ts = mn; r.max_ts = mx; r.pad = 0;
      srec[si] = r;
    }
  }
  int nk = 0;
  for (int u0 = 0; u0 < m; u0 += 64) {
    const int u = u0 + l;
    bool keep = false;
    AidRec r;
    if (u < m) {
      const int32_t a = ua[u];
      int r_ts = 1, r_n = 1, r_nc = 1, r_no = 1, r_t[3] = {1, 1, 1};
      int amin = INT32_MAX, amax = INT32_MIN;  // :190-191 over max_ts_aid of every distinct aid (before the filter)
      const bool has[3] = {un[1][u] > 0, un[2][u] > 0, un[3][u] > 0};
      for (int v = 0; v < m; ++v) {
        const int32_t b = ua[v];
        r_ts += rank_before(ut[0][v], b, ut[0][u], a);
        r_n += rank_before(un[0][v], b, un[0][u], a);
        r_nc += rank_before(un[2][v], b, un[2][u], a);
        r_no += rank_before(un[3][v], b, un[3][u], a);
        amin = min(amin, ut[0][v]); amax = max(amax, ut[0][v]);
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (un[q + 1][v] > 0) r_t[q] += rank_before(ut[q + 1][v], b, ut[q + 1][u], a);
      }
      // :199-206 keep filter (null ranks never pass)
      keep = (has[0] && r_t[0] <= CS_NLAST) || (has[1] && r_t[1] <= CS_NLAST) ||
             (has[2] && r_t[2] <= CS_NLAST) || r_n <= CS_NLAST || r_nc <= CS_NLAST || r_no <= CS_NLAST;
      // :496-503 best order (min ignores nulls) and th = max(3, 20 - 17/19 (best - 1)) (f64 as polars)
      int best = min(r_n, r_ts);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (has[q]) best = min(best, r_t[q]);
      double th = 20.0 - (17.0 / 19.0) * (double)(best - 1);
      if (th < 3.0) th = 3.0;
      r.aid = a;
#pragma unroll
      for (int q = 0; q < 4; ++q) { r.n[q] = un[q][u]; r.mt[q] = ut[q][u] < 0 ? -1 : ut[q][u]; }
      r.r_ts = r_ts; r.r_n = r_n; r.r_nc = r_nc; r.r_no = r_no;
#pragma unroll
      for (int q = 0; q < 3; ++q) r.r_t[q] = has[q] ? r_t[q] : 0;
      // :175 ts_order_aid / max(ts_order_aid) over the session's distinct aids (= m) * 100, round(0), Int8
      r.r_rel = (int32_t)round((double)r_ts / (double)m * 100.0);
      // :193-195 (max - max_ts_aid) / max(max - min, 3600) * 100, round(0), Int8
      const int64_t span = std::max<int64_t>((int64_t)amax - (int64_t)amin, 3600);
      r.rel_pos = (int32_t)round((double)((int64_t)amax - (int64_t)ut[0][u]) / (double)span * 100.0);
      // :183-185 Kleene or, fill_null(0)
      r.lic = ((un[2][u] > 0 && un[3][u] == 0) || (has[1] && has[2] && ut[2][u] > ut[3][u])) ? 1 : 0;
      r.th = (int32_t)floor(th);  // integer rank <= th  <=>  rank <= floor(th)
    }
    const uint64_t b = __ballot(keep);
    if (keep) rec[(e0 - eb) + nk + (int)mbcnt(b)] = r;
    nk += (int)__popcll(b);
  }
  if (l == 0) n_kept[si] = (uint32_t)nk;
}

struct FoldArgs {
  const uint64_t* coff;     // handle: [S + 1]
  const int32_t* cnext;
  const int16_t* cord;
  const uint16_t* cflags;
  const int64_t* off;       // event CSR
  const AidRec* rec;
  const uint32_t* n_kept;
  const SessRec* srec;
  const int32_t* session_cl;
  const int64_t* lab_off;   // [3][S + 1] or NULL
  const int32_t* lab_aid;
  int64_t S, s_lo, n_s;
};

__device__ __forceinline__ int32_t trunc_div(int64_t a, int64_t b) { return (int32_t)((double)a / (double)b); }

__global__ __launch_bounds__(64) void k_feat_fold(FoldArgs A, CandLists L, MergedLists M, FeatVals V, FeatCols C,
                                                  int* __restrict__ err) {
  const int l = threadIdx.x;
  const int64_t si = blockIdx.x;
  if (si >= A.n_s) return;
  const int64_t s = A.s_lo + si;
  const uint64_t c0 = A.coff[s], c1 = A.coff[s + 1], cb = A.coff[A.s_lo];
  const int64_t eb = A.off[A.s_lo];
  const AidRec* __restrict__ recs = A.rec + (A.off[s] - eb);
  const uint32_t nk = A.n_kept[si];
  const SessRec S = A.srec[si];
  const int32_t cl = A.session_cl ? A.session_cl[s] : -1;
  const bool has_cl = cl >= 0 && cl < L.n_clusters;
  const uint32_t pb = has_cl ? L.pop_off[cl] : 0u, pe = has_cl ? L.pop_off[cl + 1] : 0u;

  for (uint64_t t0 = c0; t0 < c1; t0 += 64) {
    const uint64_t ci = t0 + (uint64_t)l;
    const bool valid = ci < c1;
    const uint32_t xl = valid ? (uint32_t)A.cnext[ci] : 0u;
    const int ord = valid ? (int)A.cord[ci] : 999;
    const uint32_t fl = valid ? (uint32_t)A.cflags[ci] : 0u;
    const bool fold = valid && ord != 999;  // a popularity-only row carries 999 (:599); a kept aid's order is <= 512
    // accumulators of this lane's candidate
    int n_uniq = 0, nu[3] = {0, 0, 0}, sn[4] = {0, 0, 0, 0}, mxt[4] = {-1, -1, -1, -1};
    int64_t sum_ts = 0, sum_to = 0;
    int mn_ord = INT32_MAX, mn_rel = INT32_MAX, mn_ot[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, s_relpos = 0;
    int mn_rn = INT32_MAX, selfk = -1;
    int64_t rc[5] = {0, 0, 0, 0, 0}, rw[5][4] = {};
    int rh[5] = {0, 0, 0, 0, 0};
    int wn[2] = {0, 0}, wpos[2] = {0, 0}, wmn[2] = {INT32_MAX, INT32_MAX};
    int64_t wdist[2] = {0, 0}, wrank[2] = {0, 0};

    for (uint32_t k = 0; k < nk; ++k) {
      const AidRec R = recs[k];
      const uint32_t a = (uint32_t)R.aid;
      uint32_t cnt = 0, lo = 0;
      if (R.aid >= 0 && R.aid < M.n_items) { lo = M.eoff[R.aid]; cnt = M.pc[(int64_t)R.aid * ML_TH + (R.th & 31)]; }
      const bool sil = cnt > 0 && (uint32_t)M.mx[lo] == a;  // the self entry leads the merged list when a source lists it
      const uint32_t shift = sil ? 0u : 1u, total = cnt + shift;
      for (uint32_t p0 = 0; p0 < total; p0 += 64) {
        const uint32_t p = p0 + (uint32_t)l;
        uint32_t xv = a, bv = 0;
        if (p < total && p >= shift) { xv = (uint32_t)M.mx[lo + p - shift]; bv = (uint32_t)M.mbr[lo + p - shift] >> 8; }
        const uint32_t nb = min(64u, total - p0);
        for (uint32_t i = 0; i < nb; ++i) {
          const uint32_t x = (uint32_t)__shfl((int)xv, (int)i), bits = (uint32_t)__shfl((int)bv, (int)i);
          const bool match = fold && xl == x;
          if (__ballot(match) == 0) continue;
          // the pair (a, x) belongs to a candidate of this tile: its row in every source that lists it
          int64_t idx[CS_SRC];
#pragma unroll
          for (int q = 0; q < CS_SRC; ++q) {
            idx[q] = -1;
            if (((bits >> (q + 1)) & 1u) && L.off[q]) {
              const uint32_t b = L.off[q][a], e = L.off[q][a + 1];
              for (uint32_t j0 = b; j0 < e; j0 += 64) {
                const uint32_t j = j0 + (uint32_t)l;
                const uint64_t hit = __ballot(j < e && (uint32_t)L.nxt[q][j] == x);
                if (hit) { idx[q] = (int64_t)j0 + __builtin_ctzll(hit); break; }
              }
            }
          }
          if (match) {
            n_uniq += 1;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              nu[q] += R.n[q + 1] > 0;
              if (R.r_t[q] > 0) mn_ot[q] = min(mn_ot[q], R.r_t[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) { sn[q] += R.n[q]; mxt[q] = max(mxt[q], R.mt[q]); }
            sum_ts += R.mt[0];
            if (R.mt[3] >= 0) sum_to += R.mt[3];
            mn_ord = min(mn_ord, R.r_ts); mn_rel = min(mn_rel, R.r_rel); mn_rn = min(mn_rn, R.r_n);
            s_relpos += R.rel_pos;
            if (x == a) selfk = (int)k;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
              if (idx[q] >= 0) {
                const int64_t c = V.count[q][idx[q]];
                rh[q] += 1; rc[q] += c;
                rw[q][0] += c * (int64_t)V.count_pop[q][idx[q]];
                rw[q][1] += c * (int64_t)V.perc_pop[q][idx[q]];
                rw[q][2] += c * (int64_t)L.rank[q][idx[q]];
                rw[q][3] += c * (int64_t)V.count_rel[q][idx[q]];
              }
            }
#pragma unroll
            for (int w = 0; w < 2; ++w) {
              if (idx[5 + w] >= 0) {
                const int r = L.rank[5 + w][idx[5 + w]];
                wn[w] += 1; wpos[w] += r > 0; wmn[w] = min(wmn[w], r);
                wrank[w] += r; wdist[w] += V.dist[w][idx[5 + w]];
              }
            }
          }
        }
      }
    }
    if (!valid) continue;
    const uint64_t o = ci - cb;
    put<C_session>(C, o, (int32_t)s);
    put<C_aid_next>(C, o, (int32_t)xl);
    put<C_src_any>(C, o, 1);
    put<C_src_self>(C, o, (int32_t)(fl & 1u));
    put<C_src_click_to_click>(C, o, (int32_t)((fl >> 1) & 1u));
    put<C_src_click_to_cart_or_buy>(C, o, (int32_t)((fl >> 2) & 1u));
    put<C_src_cart_to_cart>(C, o, (int32_t)((fl >> 3) & 1u));
    put<C_src_cart_to_buy>(C, o, (int32_t)((fl >> 4) & 1u));
    put<C_src_buy_to_buy>(C, o, (int32_t)((fl >> 5) & 1u));
    put<C_src_w2vec_all>(C, o, (int32_t)((fl >> 6) & 1u));
    put<C_src_w2vec_1_2>(C, o, (int32_t)((fl >> 7) & 1u));
    put<C_src_pop_cl50>(C, o, (int32_t)((fl >> 8) & 1u));
    // :571-585 the six cl50 ranks of a candidate in the session's filtered cluster list
    {
      int64_t pj = -1;
      if ((fl >> 8) & 1u)
        for (uint32_t j = pb; j < pe; ++j)
          if ((uint32_t)L.pop_aid[j] == xl) { pj = j; break; }
      const int16_t* r6 = (pj >= 0 && V.pop_ranks6) ? V.pop_ranks6 + pj * 6 : nullptr;
      put<C_rank_clicks_cl50>(C, o, r6 ? r6[0] : -1);
      put<C_rank_carts_cl50>(C, o, r6 ? r6[1] : -1);
      put<C_rank_orders_cl50>(C, o, r6 ? r6[2] : -1);
      put<C_rank_clicks_7d_cl50>(C, o, r6 ? r6[3] : -1);
      put<C_rank_carts_7d_cl50>(C, o, r6 ? r6[4] : -1);
      put<C_rank_orders_7d_cl50>(C, o, r6 ? r6[5] : -1);
    }
    // :588-590 the cl1 ranks by aid_next
    {
      const int16_t* r3 = (V.cl1_ranks3 && xl < (uint32_t)L.n_items) ? V.cl1_ranks3 + (int64_t)xl * 3 : nullptr;
      put<C_rank_clicks_cl1>(C, o, r3 ? r3[0] : -1);
      put<C_rank_carts_cl1>(C, o, r3 ? r3[1] : -1);
      put<C_rank_orders_cl1>(C, o, r3 ? r3[2] : -1);
    }
    // :630-644 targets
    {
      int tg[3] = {0, 0, 0};
      if (A.lab_off) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int64_t lb = A.lab_off[t * (A.S + 1) + s], le = A.lab_off[t * (A.S + 1) + s + 1];
          for (int64_t j = lb; j < le; ++j)
            if ((uint32_t)A.lab_aid[j] == xl) { tg[t] = 1; break; }
        }
      }
      put<C_target_clicks>(C, o, tg[0]);
      put<C_target_carts>(C, o, tg[1]);
      put<C_target_orders>(C, o, tg[2]);
    }
    const bool ok = fold && n_uniq > 0;
    if (fold && n_uniq == 0) atomicOr(err, 16);  // the handle was not made from these inputs
    if (!ok) {  // popularity-only candidate: every fold, time and session column is null (:585 outer join)
      put<C_ts_order_aid>(C, o, fold ? -1 : 999);
#define NULLCOL(n) put<C_##n>(C, o, -1);
#define NULLRULE(R) NULLCOL(R##_count) NULLCOL(R##_count_pop) NULLCOL(R##_perc_pop) NULLCOL(R##_rank) NULLCOL(R##_count_rel)
#define NULLW2V(W) NULLCOL(n_w2vec_##W) NULLCOL(dist_w2vec_##W) NULLCOL(rank_w2vec_##W) NULLCOL(best_rank_w2vec_##W)
      NULLCOL(slf_n) NULLCOL(slf_n_clicks) NULLCOL(slf_n_carts) NULLCOL(slf_n_orders) NULLCOL(slf_rank_by_n)
      NULLCOL(slf_rank_by_n_carts) NULLCOL(slf_rank_by_n_orders) NULLCOL(slf_ts_rel_pos_in_session)
      NULLCOL(slf_ts_order) NULLCOL(slf_ts_order_rel) NULLCOL(slf_ts_order_clicks) NULLCOL(slf_ts_order_carts)
      NULLCOL(slf_ts_order_orders) NULLCOL(slf_left_in_cart) NULLCOL(n_uniq_aid) NULLCOL(n_uniq_aid_clicks)
      NULLCOL(n_uniq_aid_carts) NULLCOL(n_uniq_aid_orders) NULLCOL(n_aid) NULLCOL(n_aid_clicks) NULLCOL(n_aid_carts)
      NULLCOL(n_aid_orders) NULLCOL(ts_order_aid_rel) NULLCOL(ts_order_aid_clicks) NULLCOL(ts_order_aid_carts)
      NULLCOL(ts_order_aid_orders) NULLCOL(ts_aid_rel_pos_in_session) NULLCOL(rank_by_n_aid)
      NULLRULE(click_to_click) NULLRULE(click_to_cart_or_buy) NULLRULE(cart_to_cart) NULLRULE(cart_to_buy)
      NULLRULE(buy_to_buy) NULLW2V(all) NULLW2V(1_2)
      NULLCOL(n_events_session) NULLCOL(n_aids_session) NULLCOL(n_clicks_session) NULLCOL(n_carts_session)
      NULLCOL(n_orders_session) NULLCOL(duration_session) NULLCOL(only_orders_session)
      NULLCOL(since_ts_aid) NULLCOL(since_ts_aid_clicks) NULLCOL(since_ts_aid_carts) NULLCOL(since_ts_aid_orders)
      NULLCOL(slf_since_ts) NULLCOL(slf_since_ts_clicks) NULLCOL(slf_since_ts_carts) NULLCOL(slf_since_ts_orders)
      NULLCOL(since_session_start_ts_aid) NULLCOL(since_session_start_ts_aid_orders)
      NULLCOL(rel_pos_max_ts_aid_in_session) NULLCOL(rel_pos_mean_max_ts_aid_in_session)
      NULLCOL(rel_pos_mean_max_ts_aid_orders_in_session)
#undef NULLW2V
#undef NULLRULE
#undef NULLCOL
      continue;
    }
    // ---- feats_self (:309-334): at most one row of the group is the self row; a non-self row contributes
    // 0 where its column is non-null
    const bool slf = selfk >= 0;
    AidRec Rs;
    if (slf) Rs = recs[selfk];
    const int nn = n_uniq - (slf ? 1 : 0);  // non-self rows
    int nnt[3];  // non-self rows whose per-type columns are non-null
#pragma unroll
    for (int q = 0; q < 3; ++q) nnt[q] = nu[q] - ((slf && Rs.n[q + 1] > 0) ? 1 : 0);
    put<C_slf_n>(C, o, slf ? Rs.n[0] : 0);
    put<C_slf_n_clicks>(C, o, slf ? Rs.n[1] : 0);
    put<C_slf_n_carts>(C, o, slf ? Rs.n[2] : 0);
    put<C_slf_n_orders>(C, o, slf ? Rs.n[3] : 0);
    put<C_slf_rank_by_n>(C, o, nn > 0 ? 0 : Rs.r_n);
    put<C_slf_rank_by_n_carts>(C, o, nn > 0 ? 0 : Rs.r_nc);
    put<C_slf_rank_by_n_orders>(C, o, nn > 0 ? 0 : Rs.r_no);
    put<C_slf_ts_rel_pos_in_session>(C, o, nn > 0 ? 0 : Rs.rel_pos);
    put<C_slf_ts_order>(C, o, nn > 0 ? 0 : Rs.r_ts);
    put<C_slf_ts_order_rel>(C, o, nn > 0 ? 0 : Rs.r_rel);
    int so[3], smt[4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      so[q] = nnt[q] > 0 ? 0 : ((slf && Rs.r_t[q] > 0) ? Rs.r_t[q] : -1);
      smt[q + 1] = (slf && Rs.mt[q + 1] >= 0) ? Rs.mt[q + 1] : (nnt[q] > 0 ? 0 : -1);  // 0-based maximum
    }
    smt[0] = slf ? Rs.mt[0] : 0;
    put<C_slf_ts_order_clicks>(C, o, so[0]);
    put<C_slf_ts_order_carts>(C, o, so[1]);
    put<C_slf_ts_order_orders>(C, o, so[2]);
    put<C_slf_left_in_cart>(C, o, slf ? Rs.lic : 0);
    // ---- aggs_events_session (:337-364)
    put<C_n_uniq_aid>(C, o, n_uniq);
    put<C_n_uniq_aid_clicks>(C, o, nu[0]);
    put<C_n_uniq_aid_carts>(C, o, nu[1]);
    put<C_n_uniq_aid_orders>(C, o, nu[2]);
    put<C_n_aid>(C, o, sn[0]);
    put<C_n_aid_clicks>(C, o, sn[1]);
    put<C_n_aid_carts>(C, o, sn[2]);
    put<C_n_aid_orders>(C, o, sn[3]);
    put<C_ts_order_aid>(C, o, mn_ord);
    put<C_ts_order_aid_rel>(C, o, mn_rel);
    put<C_ts_order_aid_clicks>(C, o, nu[0] > 0 ? mn_ot[0] : -1);
    put<C_ts_order_aid_carts>(C, o, nu[1] > 0 ? mn_ot[1] : -1);
    put<C_ts_order_aid_orders>(C, o, nu[2] > 0 ? mn_ot[2] : -1);
    put<C_ts_aid_rel_pos_in_session>(C, o, trunc_div(s_relpos, n_uniq));
    put<C_rank_by_n_aid>(C, o, mn_rn);
    const int32_t mean_ts = trunc_div(sum_ts, n_uniq);
    const bool has_o = nu[2] > 0;
    const int32_t mean_to = has_o ? trunc_div(sum_to, nu[2]) : -1;
    // ---- aggs_counts_co_events (:367-376)
    int32_t rv[5][5];
    bool ovf = false;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      if (rh[q] == 0) {
#pragma unroll
        for (int f = 0; f < 5; ++f) rv[q][f] = -1;
        continue;
      }
      if (rc[q] > (int64_t)INT32_MAX || rc[q] < (int64_t)INT32_MIN) ovf = true;
      rv[q][0] = (int32_t)rc[q];
#pragma unroll
      for (int f = 0; f < 4; ++f) rv[q][1 + f] = rc[q] != 0 ? trunc_div(rw[q][f], rc[q]) : -1;
    }
    if (ovf) atomicOr(err, 8);
#define PUTRULE(q, R)                                                                                       \
  put<C_##R##_count>(C, o, rv[q][0]); put<C_##R##_count_pop>(C, o, rv[q][1]); put<C_##R##_perc_pop>(C, o, rv[q][2]); \
  put<C_##R##_rank>(C, o, rv[q][3]); put<C_##R##_count_rel>(C, o, rv[q][4]);
    PUTRULE(0, click_to_click) PUTRULE(1, click_to_cart_or_buy) PUTRULE(2, cart_to_cart) PUTRULE(3, cart_to_buy)
    PUTRULE(4, buy_to_buy)
#undef PUTRULE
    // ---- aggs_w2vec (:379-389)
#define PUTW2V(w, W)                                                                       \
  put<C_n_w2vec_##W>(C, o, wn[w] ? wpos[w] : -1);                                          \
  put<C_dist_w2vec_##W>(C, o, wn[w] ? trunc_div(wdist[w], wn[w]) : -1);                    \
  put<C_rank_w2vec_##W>(C, o, wn[w] ? trunc_div(wrank[w], wn[w]) : -1);                    \
  put<C_best_rank_w2vec_##W>(C, o, wn[w] ? wmn[w] : -1);
    PUTW2V(0, all) PUTW2V(1, 1_2)
#undef PUTW2V
    // ---- session statistics (:115-135, joined at :523)
    put<C_n_events_session>(C, o, S.n_events);
    put<C_n_aids_session>(C, o, S.n_aids);
    put<C_n_clicks_session>(C, o, S.n_type[0]);
    put<C_n_carts_session>(C, o, S.n_type[1]);
    put<C_n_orders_session>(C, o, S.n_type[2]);
    put<C_duration_session>(C, o, S.max_ts - S.min_ts);
    put<C_only_orders_session>(C, o, (S.n_type[0] == 0 && S.n_type[1] == 0 && S.n_type[2] > 0) ? 1 : 0);
    // ---- time columns (:526-551)
    put<C_since_ts_aid>(C, o, S.max_ts - mxt[0]);
    put<C_since_ts_aid_clicks>(C, o, nu[0] > 0 ? S.max_ts - mxt[1] : -1);
    put<C_since_ts_aid_carts>(C, o, nu[1] > 0 ? S.max_ts - mxt[2] : -1);
    put<C_since_ts_aid_orders>(C, o, nu[2] > 0 ? S.max_ts - mxt[3] : -1);
    put<C_slf_since_ts>(C, o, S.max_ts - smt[0]);
    put<C_slf_since_ts_clicks>(C, o, smt[1] >= 0 ? S.max_ts - smt[1] : -1);
    put<C_slf_since_ts_carts>(C, o, smt[2] >= 0 ? S.max_ts - smt[2] : -1);
    put<C_slf_since_ts_orders>(C, o, smt[3] >= 0 ? S.max_ts - smt[3] : -1);
    put<C_since_session_start_ts_aid>(C, o, mxt[0] - S.min_ts);
    put<C_since_session_start_ts_aid_orders>(C, o, has_o ? mxt[3] - S.min_ts : -1);
    const double span = (double)((int64_t)S.max_ts - (int64_t)S.min_ts + 1);
    put<C_rel_pos_max_ts_aid_in_session>(C, o, (int32_t)((double)((int64_t)mxt[0] - S.min_ts) / span * 100.0));
    put<C_rel_pos_mean_max_ts_aid_in_session>(C, o, (int32_t)((double)((int64_t)mean_ts - S.min_ts) / span * 100.0));
    put<C_rel_pos_mean_max_ts_aid_orders_in_session>(
        C, o, has_o ? (int32_t)((double)((int64_t)mean_to - S.min_ts) / span * 100.0) : -1);
  }
}

}  // namespace ottohip

using namespace ottohip;

extern "C" {

int ottohip_feature_columns(int i, const char** name, int* dtype) {
  if (i >= 0 && i < N_FEAT_COLS) {
    if (name) *name = kFeatNames[i];
    if (dtype) *dtype = kFeatDtype[i];
  }
  return N_FEAT_COLS;
}

int ottohip_candidates_features(ottohip_ctx* ctx, const ottohip_candidates* c, const int64_t* session_offsets,
                                const int32_t* aid, const int32_t* ts, const int8_t* type,
                                const ottohip_cand_lists* lists, const ottohip_feat_values* values,
                                const int32_t* session_cl, const int64_t* lab_off, const int32_t* lab_aid,
                                int64_t s_lo, int64_t s_hi, void* const* cols, int n_cols, void* stream) {
  if (!ctx || !c || !lists || !values || !cols || s_lo < 0 || s_hi < s_lo || s_hi > c->n_sessions ||
      (n_cols != N_FEAT_COLS && n_cols != N_FEAT_COLS - 3) ||
      (c->n_sessions > 0 && (!session_offsets || !aid || !ts || !type))) {
    set_error("candidates_features: bad arguments"); return OTTOHIP_EINVAL;
  }
  const int64_t ns = s_hi - s_lo;
  if (ns == 0) return 0;
  hipStream_t s = S(stream);
  OH_HIP(hipSetDevice(ctx->device));
  CandLists L;
  OH_TRY(cand_lists_from_abi(lists, &L, "candidates_features"));
  FeatVals V;
  for (int q = 0; q < 5; ++q) {
    V.count[q] = values->count[q]; V.count_pop[q] = values->count_pop[q];
    V.perc_pop[q] = values->perc_pop[q]; V.count_rel[q] = values->count_rel[q];
    if (L.off[q] && (!V.count[q] || !V.count_pop[q] || !V.perc_pop[q] || !V.count_rel[q])) {
      set_error("candidates_features: values of list %d incomplete", q); return OTTOHIP_EINVAL;
    }
  }
  for (int w = 0; w < 2; ++w) {
    V.dist[w] = values->dist[w];
    if (L.off[5 + w] && !V.dist[w]) { set_error("candidates_features: dist of list %d missing", 5 + w); return OTTOHIP_EINVAL; }
  }
  V.pop_ranks6 = values->pop_ranks6;
  V.cl1_ranks3 = values->cl1_ranks3;
  FeatCols C;
  for (int i = 0; i < N_FEAT_COLS; ++i) C.p[i] = i < n_cols ? cols[i] : nullptr;
  C.p[C_cos_sim_ses_aid] = nullptr;  // ottohip_session_item_similarity's columns
  C.p[C_eucl_dist_ses_aid] = nullptr;
  int64_t eo[2] = {0, 0};
  OH_TRY(d2h(&eo[0], session_offsets + s_lo, 1, s));
  OH_TRY(d2h(&eo[1], session_offsets + s_hi, 1, s));
  const int64_t E = eo[1] - eo[0];
  if (E < 0) { set_error("candidates_features: session offsets decrease"); return OTTOHIP_EINVAL; }
  Workspace& ws = ctx->ws;
  AidRec* rec;
  SessRec* srec;
  uint32_t* n_kept;
  int* err;
  OH_TRY(ws.get("ft_rec", (size_t)std::max<int64_t>(E, 1), &rec));
  OH_TRY(ws.get("ft_srec", (size_t)ns, &srec));
  OH_TRY(ws.get("ft_nkept", (size_t)ns, &n_kept));
  OH_TRY(ws.get("ft_err", 1, &err));
  OH_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
  MergedLists M;
  OH_TRY(build_merged_lists(ctx, L, &M, err, s, "candidates_features"));
  int ph = ctx->begin("feat_aids", s, 9.0 * E);
  k_feat_aids<<<(unsigned)ns, 64, 0, s>>>(session_offsets, s_lo, ns, aid, ts, type, rec, n_kept, srec, err);
  ctx->end(ph, s);
  FoldArgs A;
  A.coff = c->off; A.cnext = c->next; A.cord = c->ord; A.cflags = c->flags;
  A.off = session_offsets; A.rec = rec; A.n_kept = n_kept; A.srec = srec; A.session_cl = session_cl;
  A.lab_off = (n_cols == N_FEAT_COLS) ? lab_off : nullptr; A.lab_aid = lab_aid;
  A.S = c->n_sessions; A.s_lo = s_lo; A.n_s = ns;
  ph = ctx->begin("feat_fold", s, 0);
  k_feat_fold<<<(unsigned)ns, 64, 0, s>>>(A, L, M, V, C, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr & 1) { set_error("candidates_features: a session has more than %d events", CS_MAXE); return OTTOHIP_ELIMIT; }
  if (herr & 2) { set_error("candidates_features: a ts below 0 or a type outside {0, 1, 2}"); return OTTOHIP_ERANGE; }
  if (herr & 4) { set_error("candidates_features: an aid has more than %d list entries", ML_MAX); return OTTOHIP_ELIMIT; }
  if (herr & 16) { set_error("candidates_features: the handle was not generated from these events and lists"); return OTTOHIP_EINVAL; }
  if (herr & 8) { set_error("candidates_features: a {rule}_count sum does not fit int32"); return OTTOHIP_ELIMIT; }
  return 0;
}

}  // extern "C"
