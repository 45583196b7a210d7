// LambdaRank GBDT training (model/train_lgbm_rankers.py) on gfx950: the stages of one boosting iteration. Plain HIP:
// no inline assembly in this unit. The unit is compiled with -ffp-contract=off (csrc/Makefile): every float64
// result below is the IEEE result of the written + - * / in the written order, so tests/train_oracle.py (numpy)
// reproduces it bit for bit. There is no floating-point atomic and no device transcendental here: exp and log2
// arrive as host-built float64 tables (ottohip_train_tables), frexp / ldexp / rint / floor are exact.
//
//   k_tr_bin     a lane owns a row of one column: the value as float64, lower bound over the feature's boundaries
//                (bin = boundaries below the value), one byte into the row-major binned matrix [n][stride].
//   k_tr_grad    one workgroup per session. The rows' scores are ranked by counting (rows that sort before: larger
//                score, or equal score and earlier row: the stable descending sort, -0.0 == 0.0), the sorted score,
//                label and row sit in LDS (TR_LDS_ROWS rows at most, 21 B a row) or, above the switch, in a global
//                scratch. A lane owns a sorted position r and walks its partners in ascending position p (all p for
//                r < truncation, else p < truncation), which is the order LightGBM's double loop reaches a row in.
//                Lane 0 adds the rows' lambda sums in position order; the norm factor scales the session's g and h.
//   k_tr_absmax / k_tr_quant   max |g|, max |h| as integer maxima of the float64 bit patterns (non-negative doubles
//                order as their bits); q = rint(ldexp(x, 15 - e)) with max = m * 2^e, packed (q_g, q_h) int32 pairs.
//   k_tr_hist    a workgroup owns TR_HF drawn features (24 KB of int32 LDS bins: q_g, q_h, count) and walks chunks of
//                the row list; a lane takes one (row, feature) item: the row's 8-byte (q_g, q_h), one byte of the
//                row's bin record, three LDS integer atomics. The partials go to the int64 global histogram by
//                integer atomics after at most 2^15 rows (|q| <= 2^15, so an int32 bin holds at most 2^30) and at
//                the end. Integer sums are order-independent: the histogram is exact.
//   k_tr_scan    one workgroup per (leaf, drawn feature): the bins' prefix sums in int64, the gain of "bin <= b" in
//                float64 from the scaled sums, the best b (larger gain, then smaller b) in one record of 8 words.
//   k_tr_pcount / k_tr_pscatter   stable partition of a row list by bin <= b: per 256-row tile the count of left
//                rows, scanned; each row lands at its tile's base plus its ballot prefix. Left rows first.
//   k_tr_apply   a lane owns a row: walks the tree on the binned matrix, score += the leaf's value.
//   k_tr_ndcg    one wave per session: rank by counting, the top k gains * discounts to LDS slots, lane 0 adds them
//                in position order.
//   trainer      ottohip_trainer_*: the boosting loop on the host side of this unit. The tree's feature draw, the leaf
//                pick from the split records, the row-list segments (a leaf is [begin, begin + count) of one int32
//                buffer) and the tree's arrays; per split the host reads the children's 2 k records once, the larger
//                child's histogram is parent - smaller (k_tr_sub, int64). Host float64 (leaf values) is compiled
//                without contraction like the device code.
#include "prims.h"
#include "table.h"

#include <algorithm>
#include <cmath>

namespace ottohip {

constexpr int TR_T = 256, TR_WAVES = TR_T / 64;
// the gradient kernel's path switch: 2048 rows * (8 score + 8 lambda sum + 4 row + 1 label) = 43 KB of the 64 KB a
// workgroup may hold statically, three sessions resident per CU (160 KB); larger sessions use the global scratch
constexpr int TR_LDS_ROWS = 2048;
constexpr int TR_MAX_SESSION = 10000;  // LightGBM's query limit; the discount table's length
constexpr int TR_MAX_LABEL = 30;
constexpr int TR_BINS = 256;
constexpr int TR_HF = 8;               // drawn features per histogram workgroup (a power of two)
constexpr int TR_CHUNK = 4096;         // rows of one pass of a histogram workgroup
constexpr int TR_FLUSH_ROWS = 1 << 15; // rows a workgroup may add before its int32 partials are flushed
constexpr int TR_NDCG_K = 64;          // eval_at of the metric kernel at most
constexpr int TR_REC = 8;              // words of a split record

enum { TR_ERR_SESSION = 1, TR_ERR_LABEL = 2, TR_ERR_BIG = 4, TR_ERR_INDEX = 8, TR_ERR_SCORE = 16 };

__device__ __forceinline__ double tr_sigmoid(double d, const ottohip_train_tables& T) {
  if (d <= T.sig_min) return T.sig[0];
  if (d >= T.sig_max) return T.sig[T.n_sig - 1];
  int64_t i = (int64_t)((d - T.sig_min) * T.sig_factor);
  if (i > T.n_sig - 1) i = T.n_sig - 1;
  if (i < 0) i = 0;  // a NaN score only
  return T.sig[i];
}

// LOG2(x), x >= 1: linear interpolation of L[i] = log2(0.5 + i / 8192) on the mantissa of frexp
__device__ __forceinline__ double tr_log2(double x, const double* __restrict__ L) {
  int e;
  const double m = frexp(x, &e);
  const double t = (m - 0.5) * 8192.0;
  const double fi = floor(t);
  const int i = fi >= 0.0 && fi <= 4095.0 ? (int)fi : 0;  // outside only for a sum that is not finite
  const double f = t - fi;
  return ((double)e + L[i]) + f * (L[i + 1] - L[i]);
}

// ---------------------------------------------------------------- bins
template <class V>
__global__ __launch_bounds__(TR_T) void k_tr_bin(const V* __restrict__ col, int64_t n, const double* __restrict__ bounds,
                                                 int n_bounds, uint8_t* __restrict__ out, int stride) {
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_T) {
    const double v = (double)col[i];
    int lo = 0, hi = n_bounds;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bounds[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    out[i * stride] = (uint8_t)lo;
  }
}

// ---------------------------------------------------------------- gradients
// the session [a, a + n) with its sorted arrays ss / sl / si and the lambda sums sa (LDS or global scratch)
__device__ __forceinline__ void tr_session(const double* __restrict__ score, const int8_t* __restrict__ label,
                                           int64_t a, int n, int64_t s, double* ss, double* sa, int32_t* si,
                                           uint8_t* sl, const ottohip_train_tables& T, double* __restrict__ g,
                                           double* __restrict__ h, double* l_sum, int* __restrict__ err) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += TR_T) sa[i] = score[a + i];
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < n; i += TR_T) {
    const double x = sa[i];
    bad |= x != x ? 1 : 0;
    int rk = 0;
    for (int j = 0; j < n; ++j) {
      const double y = sa[j];
      rk += (y > x || (y == x && j < i)) ? 1 : 0;
    }
    int lab = label[a + i];
    if (lab < 0 || lab > TR_MAX_LABEL) {
      atomicOr(err, TR_ERR_LABEL);
      lab = 0;
    }
    if (rk >= n) rk = n - 1;
    ss[rk] = x;
    si[rk] = i;
    sl[rk] = (uint8_t)lab;
  }
  // a NaN score makes ranks collide and leaves slots of the sorted arrays unwritten: the session is reported and
  // skipped (g and h stay 0), nothing is read from those slots
  if (__syncthreads_or(bad)) {
    if (tid == 0) atomicOr(err, TR_ERR_SCORE);
    return;
  }
  const double best = ss[0], worst = ss[n - 1];
  const bool nz = T.norm != 0 && best != worst;
  const double inv = T.inv_max_dcg[s];
  const double sigma = T.sigma, sigma2 = T.sigma * T.sigma;
  const int trunc = T.truncation_level < n ? T.truncation_level : n;
  for (int r = tid; r < n; r += TR_T) {
    const int lr = sl[r];
    const double sr = ss[r], dr = T.disc[r], gr = T.gain[lr];
    double gg = 0.0, hh = 0.0, aa = 0.0;
    const int pend = r < trunc ? n : trunc;
    for (int p = 0; p < pend; ++p) {
      const int lp = sl[p];
      if (p == r || lp == lr) continue;
      const double sp = ss[p];
      const bool hi = lr > lp;
      const double d = hi ? sr - sp : sp - sr;
      const double dg = hi ? gr - T.gain[lp] : T.gain[lp] - gr;
      double w = (dg * fabs(dr - T.disc[p])) * inv;
      if (nz) w = w / (0.01 + fabs(d));
      const double pr = tr_sigmoid(d, T);
      const double lam = pr * (sigma * w);
      const double hes = (pr * (1.0 - pr)) * (sigma2 * w);
      gg = hi ? gg - lam : gg + lam;
      hh += hes;
      aa += lam;
    }
    const int64_t o = a + si[r];
    g[o] = gg;
    h[o] = hh;
    sa[r] = aa;  // sa's scores were last read before the barrier above
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int r = 0; r < n; ++r) sum += sa[r];
    *l_sum = sum;
  }
  __syncthreads();
  const double sum = *l_sum;
  if (T.norm != 0 && sum > 0.0) {
    const double f = tr_log2(1.0 + sum, T.log2t) / sum;
    for (int r = tid; r < n; r += TR_T) {
      const int64_t o = a + si[r];
      g[o] = g[o] * f;
      h[o] = h[o] * f;
    }
  }
}

// big == 0: the sessions up to TR_LDS_ROWS rows (larger ones are flagged); big == 1: only the larger ones, in scratch
__global__ __launch_bounds__(TR_T) void k_tr_grad(const double* __restrict__ score, const int8_t* __restrict__ label,
                                                  const int64_t* __restrict__ off, int64_t S, int64_t n_rows,
                                                  const ottohip_train_tables T, double* __restrict__ g,
                                                  double* __restrict__ h, int big, double* g_ss, double* g_sa,
                                                  int32_t* g_si, uint8_t* g_sl, int* __restrict__ err) {
  __shared__ double l_ss[TR_LDS_ROWS];
  __shared__ double l_sa[TR_LDS_ROWS];
  __shared__ int32_t l_si[TR_LDS_ROWS];
  __shared__ uint8_t l_sl[TR_LDS_ROWS];
  __shared__ double l_sum;
  const int64_t s = blockIdx.x;
  if (s >= S) return;
  const int64_t o0 = off[0];
  const int64_t a = min(max(off[s] - o0, (int64_t)0), n_rows);
  const int64_t b = min(max(off[s + 1] - o0, a), n_rows);
  const int64_t n = b - a;
  if (n == 0) return;
  if (n > TR_MAX_SESSION) {  // block-uniform
    if (threadIdx.x == 0) atomicOr(err, TR_ERR_SESSION);
    return;
  }
  if (n <= TR_LDS_ROWS) {
    if (big) return;
    tr_session(score, label, a, (int)n, s, l_ss, l_sa, l_si, l_sl, T, g, h, &l_sum, err);
  } else {
    if (!big) {
      if (threadIdx.x == 0) atomicOr(err, TR_ERR_BIG);
      return;
    }
    tr_session(score, label, a, (int)n, s, g_ss + a, g_sa + a, g_si + a, g_sl + a, T, g, h, &l_sum, err);
  }
}

// ---------------------------------------------------------------- quantiser
__global__ __launch_bounds__(TR_T) void k_tr_absmax(const double* __restrict__ g, const double* __restrict__ h, int64_t n,
                                                    unsigned long long* __restrict__ mx) {
  unsigned long long mg = 0, mh = 0;
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_T) {
    const unsigned long long bg = (unsigned long long)__double_as_longlong(fabs(g[i]));
    const unsigned long long bh = (unsigned long long)__double_as_longlong(fabs(h[i]));
    mg = bg > mg ? bg : mg;
    mh = bh > mh ? bh : mh;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long og = shfl64(mg, (int)(lane_id() ^ (uint32_t)d));
    const unsigned long long oh = shfl64(mh, (int)(lane_id() ^ (uint32_t)d));
    mg = og > mg ? og : mg;
    mh = oh > mh ? oh : mh;
  }
  if (lane_id() == 0u) {
    atomicMax(&mx[0], mg);
    atomicMax(&mx[1], mh);
  }
}

// info: {e_g, e_h, max|g| == 0}
__global__ __launch_bounds__(TR_T) void k_tr_quant(const double* __restrict__ g, const double* __restrict__ h, int64_t n,
                                                   const unsigned long long* __restrict__ mx, int2* __restrict__ gh,
                                                   int* __restrict__ info) {
  const double maxg = __longlong_as_double((long long)mx[0]), maxh = __longlong_as_double((long long)mx[1]);
  int eg = 0, eh = 0;
  (void)frexp(maxg, &eg);
  (void)frexp(maxh, &eh);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = eg;
    info[1] = eh;
    info[2] = maxg == 0.0 ? 1 : 0;
  }
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_T)
    gh[i] = make_int2((int)rint(ldexp(g[i], 15 - eg)), (int)rint(ldexp(h[i], 15 - eh)));
}

// ---------------------------------------------------------------- histogram
__global__ __launch_bounds__(TR_T) void k_tr_hist(const uint8_t* __restrict__ bins, int stride, int64_t n_total,
                                                  const int2* __restrict__ gh, const int32_t* __restrict__ rows,
                                                  int64_t n, const int32_t* __restrict__ feats, int k,
                                                  unsigned long long* __restrict__ hist, int* __restrict__ err) {
  __shared__ int l_h[TR_HF * TR_BINS * 3];
  __shared__ int l_f[TR_HF];
  const int f0 = (int)blockIdx.y * TR_HF;
  const int nf = min(TR_HF, k - f0);
  const int tid = threadIdx.x;
  if (tid < TR_HF) {
    int f = tid < nf ? feats[f0 + tid] : -1;
    if (tid < nf && (f < 0 || f >= stride)) {
      atomicOr(err, TR_ERR_INDEX);
      f = -1;
    }
    l_f[tid] = f;
  }
  for (int i = tid; i < TR_HF * TR_BINS * 3; i += TR_T) l_h[i] = 0;
  __syncthreads();
  unsigned long long* out = hist + (size_t)f0 * TR_BINS * 3;
  int held = 0;  // rows in the LDS partials
  for (int64_t base = (int64_t)blockIdx.x * TR_CHUNK; base < n; base += (int64_t)gridDim.x * TR_CHUNK) {
    const int m = (int)min((int64_t)TR_CHUNK, n - base);
    // a lane per (row, feature) item, not per row: a lane that walks its row's nf features chains nf dependent
    // byte loads and 3 nf LDS atomics, and measured 0.73 ms against 0.39 ms for the root of 3 M rows x 26 features
    for (int idx = tid; idx < m * nf; idx += TR_T) {
      int ri, fi;
      if (nf == TR_HF) {  // a full feature group: no division
        ri = idx >> 3;
        fi = idx & (TR_HF - 1);
      } else {
        ri = idx / nf;
        fi = idx - ri * nf;
      }
      const int64_t r = rows[base + ri];
      const int f = l_f[fi];
      if (r < 0 || r >= n_total) {
        atomicOr(err, TR_ERR_INDEX);
        continue;
      }
      if (f < 0) continue;
      const int2 q = gh[r];
      int* c = &l_h[(fi * TR_BINS + (int)bins[r * stride + f]) * 3];
      atomicAdd(&c[0], q.x);
      atomicAdd(&c[1], q.y);
      atomicAdd(&c[2], 1);
    }
    held += m;
    if (held + TR_CHUNK > TR_FLUSH_ROWS) {  // block-uniform: the next chunk could pass 2^15 rows
      __syncthreads();
      for (int i = tid; i < nf * TR_BINS * 3; i += TR_T) {
        const int v = l_h[i];
        if (v) atomicAdd(&out[i], (unsigned long long)(long long)v);
        l_h[i] = 0;
      }
      __syncthreads();
      held = 0;
    }
  }
  __syncthreads();
  for (int i = tid; i < nf * TR_BINS * 3; i += TR_T) {
    const int v = l_h[i];
    if (v) atomicAdd(&out[i], (unsigned long long)(long long)v);
  }
}

// ---------------------------------------------------------------- split scan
// hist [n_hist][k][256][3]; rec [n_hist * k][8] = {gain bits, bin or -1, Qg left, Qh left, count left, Qg, Qh, count}
__global__ __launch_bounds__(TR_T) void k_tr_scan(const long long* __restrict__ hist, int k,
                                                  const int32_t* __restrict__ n_bins, double sg, double sh,
                                                  long long min_child, double min_hess, double l2,
                                                  long long* __restrict__ rec) {
  __shared__ long long l_q[TR_BINS][3];
  __shared__ long long l_p[TR_BINS][3];
  __shared__ double l_gain[TR_BINS];
  const int item = blockIdx.x, b = threadIdx.x;
  const int nb = min(max(n_bins[item % k], 0), TR_BINS);
  const long long* src = hist + (size_t)item * TR_BINS * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) l_q[b][c] = src[b * 3 + c];
  __syncthreads();
  long long qg = 0, qh = 0, cn = 0;
  for (int j = 0; j <= b; ++j) {
    qg += l_q[j][0];
    qh += l_q[j][1];
    cn += l_q[j][2];
  }
  l_p[b][0] = qg;
  l_p[b][1] = qh;
  l_p[b][2] = cn;
  __syncthreads();
  const long long QG = l_p[TR_BINS - 1][0], QH = l_p[TR_BINS - 1][1], C = l_p[TR_BINS - 1][2];
  const double GL = (double)qg * sg, HL = (double)qh * sh;
  const double GR = (double)(QG - qg) * sg, HR = (double)(QH - qh) * sh;
  const double G = (double)QG * sg, H = (double)QH * sh;
  const double gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - (G * G) / (H + l2);
  const bool ok = b < nb - 1 && cn >= min_child && C - cn >= min_child && HL >= min_hess && HR >= min_hess && gain > 0.0;
  l_gain[b] = ok ? gain : -1.0;
  __syncthreads();
  if (b == 0) {
    int best = -1;
    double bg = 0.0;
    for (int j = 0; j < TR_BINS; ++j)
      if (l_gain[j] > bg) {
        bg = l_gain[j];
        best = j;
      }
    long long* o = rec + (size_t)item * TR_REC;
    o[0] = __double_as_longlong(bg);
    o[1] = best;
    o[2] = best >= 0 ? l_p[best][0] : 0;
    o[3] = best >= 0 ? l_p[best][1] : 0;
    o[4] = best >= 0 ? l_p[best][2] : 0;
    o[5] = QG;
    o[6] = QH;
    o[7] = C;
  }
}

// ---------------------------------------------------------------- partition
__global__ __launch_bounds__(TR_T) void k_tr_pcount(const uint8_t* __restrict__ bins, int stride, int64_t n_total,
                                                    int feature, int bin, const int32_t* __restrict__ rows, int64_t n,
                                                    uint32_t* __restrict__ cnt, int* __restrict__ err) {
  __shared__ uint32_t l_w[TR_WAVES];
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  bool left = false;
  if (i < n) {
    const int64_t r = rows[i];
    if (r < 0 || r >= n_total) atomicOr(err, TR_ERR_INDEX);
    else left = (int)bins[r * stride + feature] <= bin;
  }
  const uint64_t bal = __ballot(left);
  if (lane_id() == 0u) l_w[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = l_w[0] + l_w[1] + l_w[2] + l_w[3];
}

__global__ __launch_bounds__(TR_T) void k_tr_pscatter(const uint8_t* __restrict__ bins, int stride, int64_t n_total,
                                                      int feature, int bin, const int32_t* __restrict__ rows, int64_t n,
                                                      const uint64_t* __restrict__ toff,
                                                      const uint64_t* __restrict__ total, int32_t* __restrict__ out) {
  __shared__ uint32_t l_w[TR_WAVES];
  const int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x;
  const uint32_t w = threadIdx.x >> 6;
  bool left = false, live = i < n;
  int32_t r = 0;
  if (live) {
    r = rows[i];
    left = r >= 0 && r < n_total && (int)bins[(int64_t)r * stride + feature] <= bin;
  }
  const uint64_t bal = __ballot(left);
  const uint32_t pre = mbcnt(bal);
  if (lane_id() == 0u) l_w[w] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t v = 0; v < (uint32_t)TR_WAVES; ++v) before += v < w ? l_w[v] : 0u;
  if (!live) return;
  const int64_t lpos = (int64_t)toff[blockIdx.x] + before + pre;  // left rows before this one
  const int64_t pos = left ? lpos : (int64_t)total[0] + (i - lpos);
  if (pos >= 0 && pos < n) out[pos] = r;
}

// ---------------------------------------------------------------- tree apply
__global__ __launch_bounds__(TR_T) void k_tr_apply(const uint8_t* __restrict__ bins, int stride, int64_t n,
                                                   const int32_t* __restrict__ sf, const int32_t* __restrict__ sb,
                                                   const int32_t* __restrict__ lc, const int32_t* __restrict__ rc,
                                                   const double* __restrict__ lv, int n_leaves,
                                                   double* __restrict__ score, int* __restrict__ err) {
  const int ni = n_leaves - 1;
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_T) {
    int node = 0, leaf = ni == 0 ? 0 : -1;
    for (int it = 0; it < ni && leaf < 0; ++it) {
      const int f = sf[node];
      if (f < 0 || f >= stride) break;
      const int nx = (int)bins[i * stride + f] <= sb[node] ? lc[node] : rc[node];
      if (nx < 0) leaf = ~nx;
      else if (nx < ni) node = nx;
      else break;
    }
    if (leaf < 0 || leaf >= n_leaves) {
      atomicOr(err, TR_ERR_INDEX);
      continue;
    }
    score[i] = score[i] + lv[leaf];
  }
}

// ---------------------------------------------------------------- NDCG
__global__ __launch_bounds__(TR_T) void k_tr_ndcg(const double* __restrict__ score, const int8_t* __restrict__ label,
                                                  const int64_t* __restrict__ off, int64_t S, int64_t n_rows,
                                                  const double* __restrict__ gain, const double* __restrict__ disc,
                                                  const double* __restrict__ inv_max, int k, double* __restrict__ out,
                                                  int* __restrict__ err) {
  __shared__ double l_slot[TR_WAVES][TR_NDCG_K];
  const uint32_t w = threadIdx.x >> 6, l = lane_id();
  const int64_t s = (int64_t)blockIdx.x * TR_WAVES + w;
  const bool live = s < S;  // wave-uniform
  const int64_t o0 = off[0];
  const int64_t a = live ? min(max(off[s] - o0, (int64_t)0), n_rows) : 0;
  const int64_t b = live ? min(max(off[s + 1] - o0, a), n_rows) : 0;
  const int64_t n = b - a;
  l_slot[w][l] = 0.0;
  __syncthreads();
  for (int64_t i = l; i < n; i += 64) {
    const double x = score[a + i];
    int64_t rk = 0;
    for (int64_t j = 0; j < n; ++j) {
      const double y = score[a + j];
      rk += (y > x || (y == x && j < i)) ? 1 : 0;
    }
    if (rk < k) {
      int lab = label[a + i];
      if (lab < 0 || lab > TR_MAX_LABEL) {
        atomicOr(err, TR_ERR_LABEL);
        lab = 0;
      }
      l_slot[w][rk] = gain[lab] * disc[rk];
    }
  }
  __syncthreads();
  if (live && l == 0u) {
    const double inv = inv_max[s];
    double dcg = 0.0;
    const int m = (int)min((int64_t)k, n);
    for (int p = 0; p < m; ++p) dcg += l_slot[w][p];
    out[s] = inv > 0.0 ? dcg * inv : 1.0;
  }
}

static int tr_err(Ctx* ctx, hipStream_t s, int** err) {
  OH_TRY(ctx->ws.get("tr_err", 1, err));
  OH_HIP(hipMemsetAsync(*err, 0, sizeof(int), s));
  return 0;
}

}  // namespace ottohip


// ---------------------------------------------------------------- trainer handle
struct ottohip_trainer {
  ottohip_ctx* ctx = nullptr;
  const uint8_t* bins = nullptr;
  int stride = 0;
  int64_t n = 0, S = 0;
  std::vector<int> n_bins, valid;
  const int8_t* labels = nullptr;
  const int64_t* off = nullptr;
  ottohip_train_tables T{};
  ottohip_train_params P{};
  int k_max = 0;
  // device buffers (dev_alloc)
  double *scores = nullptr, *g = nullptr, *h = nullptr, *lv = nullptr, *g_ss = nullptr, *g_sa = nullptr;
  int2* gh = nullptr;
  int32_t *rows = nullptr, *tmp = nullptr, *feats = nullptr, *nb = nullptr, *tree = nullptr, *g_si = nullptr;
  uint8_t* g_sl = nullptr;
  long long *hist = nullptr, *rec = nullptr;
  unsigned long long* mx = nullptr;
  int *info = nullptr, *err = nullptr;
  bool big = false;
  int n_trees = 0;
  // the last tree (host)
  std::vector<int32_t> sf, sb, lc, rc;
  std::vector<double> sgain, ival, iwt, lval, lwt;
  std::vector<int64_t> icnt, lcnt;
};

namespace ottohip {

__global__ __launch_bounds__(TR_T) void k_tr_iota(int32_t* __restrict__ rows, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * TR_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * TR_T) rows[i] = (int32_t)i;
}

// the children's histograms from the parent's P and the smaller child's S, in place (integer: exact):
// small_is_left: P = S, S = P - S; else P = P - S (S stays). P is the left child's slot, S the right child's.
__global__ __launch_bounds__(TR_T) void k_tr_sub(long long* __restrict__ P, long long* __restrict__ Sm, int n,
                                                 int small_is_left) {
  const int i = (int)blockIdx.x * TR_T + threadIdx.x;
  if (i >= n) return;
  const long long p = P[i], s = Sm[i];
  if (small_is_left) {
    P[i] = s;
    Sm[i] = p - s;
  } else {
    P[i] = p - s;
  }
}

static uint64_t tr_mix(uint64_t z) {  // the draw of downsample.hip
  z += 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

template <class T>
static int tr_alloc(T** p, size_t n, const char* what) {
  hipError_t e = dev_alloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(T), what);
  if (e != hipSuccess) {
    set_error("trainer: allocation of %s failed: %s", what, hipGetErrorString(e));
    return OTTOHIP_ENOMEM;
  }
  return 0;
}

struct TrBest {
  bool ok = false;
  double gain = 0.0;
  int feature = 0, bin = 0;
  long long qgl = 0, qhl = 0, cl = 0;
};
struct TrLeaf {
  int64_t begin = 0, cnt = 0;
  int depth = 0, parent = -1;
  long long QG = 0, QH = 0;
  TrBest best;
};

// the best split of a leaf from its features' records: larger gain, then the smaller feature index
static TrBest tr_best(const long long* rec, const std::vector<int>& drawn) {
  TrBest b;
  for (size_t j = 0; j < drawn.size(); ++j) {
    const long long* r = rec + j * TR_REC;
    double gain;
    memcpy(&gain, &r[0], sizeof(double));
    if (r[1] >= 0 && gain > 0.0 && (!b.ok || gain > b.gain)) {
      b.ok = true; b.gain = gain; b.feature = drawn[j]; b.bin = (int)r[1];
      b.qgl = r[2]; b.qhl = r[3]; b.cl = r[4];
    }
  }
  return b;
}

static void tr_launch_hist(ottohip_trainer* t, const int32_t* rows, int64_t n, int k, long long* hist, hipStream_t s) {
  (void)hipMemsetAsync(hist, 0, (size_t)k * TR_BINS * 3 * sizeof(long long), s);
  if (n == 0) return;
  const int64_t gx = std::min<int64_t>(ceil_div(n, TR_CHUNK), (int64_t)t->ctx->n_cu * 4);
  k_tr_hist<<<dim3((unsigned)gx, (unsigned)ceil_div(k, TR_HF)), TR_T, 0, s>>>(
      t->bins, t->stride, t->n, t->gh, rows, n, t->feats, k, reinterpret_cast<unsigned long long*>(hist), t->err);
}

static void tr_launch_scan(ottohip_trainer* t, const long long* hist, int k, double sg, double sh, long long* rec,
                           hipStream_t s) {
  k_tr_scan<<<(unsigned)k, TR_T, 0, s>>>(hist, k, t->nb, sg, sh, (long long)t->P.min_child_samples,
                                         t->P.min_sum_hessian, t->P.lambda_l2, rec);
}

// grows the tree of this iteration from the quantised gradients; *n_leaves = 0: no split was found
static int tr_grow(ottohip_trainer* t, int eg, int eh, int* n_leaves, hipStream_t s) {
  *n_leaves = 0;
  const ottohip_train_params& P = t->P;
  const int nv = (int)t->valid.size();
  if (nv == 0 || t->n == 0) return 0;
  const int k = std::min(nv, std::max(1, (int)std::floor((double)nv * P.colsample_bytree + 0.5)));
  std::vector<std::pair<uint64_t, int>> keyed;
  const uint64_t sm = tr_mix(P.seed);
  for (int f : t->valid) keyed.push_back({tr_mix(sm ^ (((uint64_t)t->n_trees << 32) | (uint64_t)(uint32_t)f)), f});
  std::sort(keyed.begin(), keyed.end());
  std::vector<int> drawn;
  for (int j = 0; j < k; ++j) drawn.push_back(keyed[(size_t)j].second);
  std::sort(drawn.begin(), drawn.end());
  std::vector<int32_t> hf(drawn.begin(), drawn.end()), hnb;
  for (int f : drawn) hnb.push_back(t->n_bins[(size_t)f]);
  OH_HIP(hipMemcpyAsync(t->feats, hf.data(), (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, s));
  OH_HIP(hipMemcpyAsync(t->nb, hnb.data(), (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, s));
  OH_HIP(hipStreamSynchronize(s));  // hf / hnb are pageable host vectors
  const double sg = std::ldexp(1.0, eg - 15), sh = std::ldexp(1.0, eh - 15);
  const double l2 = P.lambda_l2, lr = P.learning_rate;
  auto value = [&](long long QG, long long QH) {
    const double H = (double)QH * sh + l2;
    return H == 0.0 ? 0.0 : (-((double)QG * sg) / H) * lr;
  };
  const size_t hsz = (size_t)t->k_max * TR_BINS * 3;  // a leaf's histogram slot
  std::vector<long long> rec((size_t)2 * k * TR_REC);
  k_tr_iota<<<(unsigned)std::min<int64_t>(ceil_div(t->n, TR_T), (int64_t)t->ctx->n_cu * 16), TR_T, 0, s>>>(t->rows, t->n);
  tr_launch_hist(t, t->rows, t->n, k, t->hist, s);
  tr_launch_scan(t, t->hist, k, sg, sh, t->rec, s);
  OH_HIP(hipGetLastError());
  OH_TRY(d2h(rec.data(), t->rec, (size_t)k * TR_REC, s));
  std::vector<TrLeaf> leaves(1);
  leaves[0].cnt = t->n;
  leaves[0].QG = rec[5]; leaves[0].QH = rec[6];
  leaves[0].best = tr_best(rec.data(), drawn);
  t->sf.clear(); t->sb.clear(); t->lc.clear(); t->rc.clear(); t->sgain.clear(); t->ival.clear(); t->iwt.clear();
  t->icnt.clear();
  for (int i = 0; i < P.num_leaves - 1; ++i) {
    int pick = -1;
    for (int L = 0; L < (int)leaves.size(); ++L) {
      const TrLeaf& lf = leaves[(size_t)L];
      if (lf.best.ok && (P.max_depth <= 0 || lf.depth < P.max_depth) &&
          (pick < 0 || lf.best.gain > leaves[(size_t)pick].best.gain))
        pick = L;
    }
    if (pick < 0) break;
    const TrLeaf lf = leaves[(size_t)pick];
    const TrBest b = lf.best;
    // stable partition of the leaf's segment; the left count is the histogram's (no read)
    const int64_t nt = ceil_div(lf.cnt, TR_T);
    uint32_t* cnt = nullptr;
    uint64_t *toff = nullptr, *total = nullptr;
    OH_TRY(t->ctx->ws.get("tr_pcnt", (size_t)nt, &cnt));
    OH_TRY(t->ctx->ws.get("tr_poff", (size_t)nt, &toff));
    OH_TRY(t->ctx->ws.get("tr_ptot", 1, &total));
    const int32_t* seg = t->rows + lf.begin;
    k_tr_pcount<<<(unsigned)nt, TR_T, 0, s>>>(t->bins, t->stride, t->n, b.feature, b.bin, seg, lf.cnt, cnt, t->err);
    OH_TRY(exclusive_scan_u32(t->ctx, cnt, toff, nt, total, s));
    k_tr_pscatter<<<(unsigned)nt, TR_T, 0, s>>>(t->bins, t->stride, t->n, b.feature, b.bin, seg, lf.cnt, toff, total,
                                                t->tmp);
    OH_HIP(hipMemcpyAsync(t->rows + lf.begin, t->tmp, (size_t)lf.cnt * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (lf.parent >= 0) {
      if (t->lc[(size_t)lf.parent] == ~pick) t->lc[(size_t)lf.parent] = i;
      else t->rc[(size_t)lf.parent] = i;
    }
    t->sf.push_back(b.feature); t->sb.push_back(b.bin); t->sgain.push_back(b.gain);
    t->lc.push_back(~pick); t->rc.push_back(~(i + 1));
    t->ival.push_back(value(lf.QG, lf.QH)); t->iwt.push_back((double)lf.QH * sh); t->icnt.push_back(lf.cnt);
    TrLeaf left, right;
    left.begin = lf.begin; left.cnt = b.cl; left.depth = lf.depth + 1; left.parent = i;
    left.QG = b.qgl; left.QH = b.qhl;
    right.begin = lf.begin + b.cl; right.cnt = lf.cnt - b.cl; right.depth = lf.depth + 1; right.parent = i;
    right.QG = lf.QG - b.qgl; right.QH = lf.QH - b.qhl;
    if (i + 1 < P.num_leaves - 1 && (P.max_depth <= 0 || left.depth < P.max_depth)) {
      long long* Pslot = t->hist + (size_t)pick * hsz;      // the parent's, then the left child's
      long long* Sslot = t->hist + (size_t)(i + 1) * hsz;   // the right child's
      const bool small_left = left.cnt <= right.cnt;
      const TrLeaf& sm_leaf = small_left ? left : right;
      tr_launch_hist(t, t->rows + sm_leaf.begin, sm_leaf.cnt, k, Sslot, s);
      const int ne = k * TR_BINS * 3;
      k_tr_sub<<<(unsigned)ceil_div(ne, TR_T), TR_T, 0, s>>>(Pslot, Sslot, ne, small_left ? 1 : 0);
      tr_launch_scan(t, Pslot, k, sg, sh, t->rec, s);
      tr_launch_scan(t, Sslot, k, sg, sh, t->rec + (size_t)k * TR_REC, s);
      OH_HIP(hipGetLastError());
      OH_TRY(d2h(rec.data(), t->rec, (size_t)2 * k * TR_REC, s));  // the one read of this split
      left.best = tr_best(rec.data(), drawn);
      right.best = tr_best(rec.data() + (size_t)k * TR_REC, drawn);
    }
    leaves[(size_t)pick] = left;
    leaves.push_back(right);
  }
  if (t->sf.empty()) return 0;
  t->lval.clear(); t->lwt.clear(); t->lcnt.clear();
  for (const TrLeaf& lf : leaves) {
    t->lval.push_back(value(lf.QG, lf.QH));
    t->lwt.push_back((double)lf.QH * sh);
    t->lcnt.push_back(lf.cnt);
  }
  *n_leaves = (int)leaves.size();
  return 0;
}

}  // namespace ottohip

using namespace ottohip;

extern "C" {

int ottohip_train_lds_rows(void) { return TR_LDS_ROWS; }

int ottohip_train_bin_column(ottohip_ctx* ctx, const void* col, int dtype, int64_t n_rows, const double* bounds,
                             int n_bounds, uint8_t* bins, int stride, int feature, void* stream) {
  if (!ctx || dtype < 0 || dtype > 3 || n_rows < 0 || n_bounds < 0 || n_bounds > TR_BINS - 1 || stride < 1 ||
      feature < 0 || feature >= stride || (n_rows > 0 && (!col || !bins)) || (n_bounds > 0 && !bounds)) {
    set_error("train_bin_column: bad arguments (dtype 0..3, 0 <= n_bounds <= %d, 0 <= feature < stride)", TR_BINS - 1);
    return OTTOHIP_EINVAL;
  }
  if (n_rows == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n_rows, TR_T), (int64_t)ctx->n_cu * 16);
  uint8_t* out = bins + feature;
  if (dtype == 0) k_tr_bin<<<grid, TR_T, 0, s>>>(static_cast<const int8_t*>(col), n_rows, bounds, n_bounds, out, stride);
  else if (dtype == 1) k_tr_bin<<<grid, TR_T, 0, s>>>(static_cast<const int16_t*>(col), n_rows, bounds, n_bounds, out, stride);
  else if (dtype == 2) k_tr_bin<<<grid, TR_T, 0, s>>>(static_cast<const int32_t*>(col), n_rows, bounds, n_bounds, out, stride);
  else k_tr_bin<<<grid, TR_T, 0, s>>>(static_cast<const float*>(col), n_rows, bounds, n_bounds, out, stride);
  OH_HIP(hipGetLastError());
  return 0;
}

int ottohip_train_gradients(ottohip_ctx* ctx, const double* scores, const int8_t* labels, const int64_t* off,
                            int64_t n_sessions, int64_t n_rows, const ottohip_train_tables* tables, double* g,
                            double* h, void* stream) {
  if (!ctx || !tables || n_sessions < 0 || n_rows < 0 || (n_sessions > 0 && !off) ||
      (n_rows > 0 && (!scores || !labels || !g || !h)) || !tables->gain || !tables->disc || !tables->sig ||
      !tables->log2t || (n_sessions > 0 && !tables->inv_max_dcg) || tables->n_sig < 2 ||
      tables->truncation_level < 1 || !(tables->sigma > 0.0)) {
    set_error("train_gradients: bad arguments (tables not NULL, n_sig >= 2, truncation_level >= 1, sigma > 0)");
    return OTTOHIP_EINVAL;
  }
  if (n_sessions >= ((int64_t)1 << 31)) {
    set_error("train_gradients: %lld sessions, a call takes fewer than 2^31", (long long)n_sessions);
    return OTTOHIP_ELIMIT;
  }
  if (n_rows == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  OH_HIP(hipMemsetAsync(g, 0, (size_t)n_rows * sizeof(double), s));
  OH_HIP(hipMemsetAsync(h, 0, (size_t)n_rows * sizeof(double), s));
  if (n_sessions == 0) return 0;
  int* err = nullptr;
  OH_TRY(tr_err(ctx, s, &err));
  ctx->reset_timing();
  int ph = ctx->begin("train_gradients", s, (double)n_rows * 25.0);
  k_tr_grad<<<(unsigned)n_sessions, TR_T, 0, s>>>(scores, labels, off, n_sessions, n_rows, *tables, g, h, 0, nullptr,
                                                  nullptr, nullptr, nullptr, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr & TR_ERR_SESSION) {
    set_error("train_gradients: a session has more than %d rows", TR_MAX_SESSION);
    return OTTOHIP_ELIMIT;
  }
  if ((herr & TR_ERR_BIG) && !(herr & (TR_ERR_LABEL | TR_ERR_SCORE))) {
    double *ss = nullptr, *sa = nullptr;
    int32_t* si = nullptr;
    uint8_t* sl = nullptr;
    OH_TRY(ctx->ws.get("tr_ss", (size_t)n_rows, &ss));
    OH_TRY(ctx->ws.get("tr_sa", (size_t)n_rows, &sa));
    OH_TRY(ctx->ws.get("tr_si", (size_t)n_rows, &si));
    OH_TRY(ctx->ws.get("tr_sl", (size_t)n_rows, &sl));
    OH_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    ph = ctx->begin("train_gradients_global", s, 0);
    k_tr_grad<<<(unsigned)n_sessions, TR_T, 0, s>>>(scores, labels, off, n_sessions, n_rows, *tables, g, h, 1, ss, sa,
                                                    si, sl, err);
    ctx->end(ph, s);
    OH_HIP(hipGetLastError());
    OH_TRY(d2h(&herr, err, 1, s));
  }
  if (herr & TR_ERR_LABEL) {
    set_error("train_gradients: a label is outside [0, %d]", TR_MAX_LABEL);
    return OTTOHIP_ERANGE;
  }
  if (herr & TR_ERR_SCORE) {
    set_error("train_gradients: a score is NaN");
    return OTTOHIP_ERANGE;
  }
  return 0;
}

int ottohip_train_quantise(ottohip_ctx* ctx, const double* g, const double* h, int64_t n_rows, int32_t* gh, int* e_g,
                           int* e_h, int* all_zero, void* stream) {
  if (!ctx || n_rows < 0 || !e_g || !e_h || !all_zero || (n_rows > 0 && (!g || !h || !gh))) {
    set_error("train_quantise: bad arguments"); return OTTOHIP_EINVAL;
  }
  *e_g = 0; *e_h = 0; *all_zero = 1;
  if (n_rows == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  unsigned long long* mx = nullptr;
  int* info = nullptr;
  OH_TRY(ctx->ws.get("tr_max", 2, &mx));
  OH_TRY(ctx->ws.get("tr_info", 4, &info));
  OH_HIP(hipMemsetAsync(mx, 0, 2 * sizeof(unsigned long long), s));
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n_rows, TR_T), (int64_t)ctx->n_cu * 8);
  ctx->reset_timing();
  const int ph = ctx->begin("train_quantise", s, (double)n_rows * 40.0);
  k_tr_absmax<<<grid, TR_T, 0, s>>>(g, h, n_rows, mx);
  k_tr_quant<<<grid, TR_T, 0, s>>>(g, h, n_rows, mx, reinterpret_cast<int2*>(gh), info);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int hinfo[3] = {0, 0, 0};
  OH_TRY(d2h(hinfo, info, 3, s));
  *e_g = hinfo[0]; *e_h = hinfo[1]; *all_zero = hinfo[2];
  return 0;
}

int ottohip_train_histogram(ottohip_ctx* ctx, const uint8_t* bins, int stride, int64_t n_total, const int32_t* gh,
                            const int32_t* rows, int64_t n, const int32_t* feats, int k, int64_t* hist, int max_blocks,
                            void* stream) {
  if (!ctx || stride < 1 || n_total < 0 || n < 0 || k < 0 || max_blocks < 0 || (k > 0 && (!feats || !hist)) ||
      (n > 0 && (!bins || !gh || !rows))) {
    set_error("train_histogram: bad arguments"); return OTTOHIP_EINVAL;
  }
  if (k == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  OH_HIP(hipMemsetAsync(hist, 0, (size_t)k * TR_BINS * 3 * sizeof(int64_t), s));
  if (n == 0) return 0;
  int* err = nullptr;
  OH_TRY(tr_err(ctx, s, &err));
  int64_t gx = std::min<int64_t>(ceil_div(n, TR_CHUNK), (int64_t)ctx->n_cu * 4);
  if (max_blocks > 0) gx = std::min<int64_t>(gx, max_blocks);
  ctx->reset_timing();
  const int ph = ctx->begin("train_histogram", s, (double)n * (12.0 + 128.0));
  k_tr_hist<<<dim3((unsigned)gx, (unsigned)ceil_div(k, TR_HF)), TR_T, 0, s>>>(
      bins, stride, n_total, reinterpret_cast<const int2*>(gh), rows, n, feats, k,
      reinterpret_cast<unsigned long long*>(hist), err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) { set_error("train_histogram: a row or feature index is outside the binned matrix"); return OTTOHIP_ERANGE; }
  return 0;
}

int ottohip_train_split_scan(ottohip_ctx* ctx, const int64_t* hist, int n_hist, int k, const int32_t* n_bins, int e_g,
                             int e_h, int64_t min_child_samples, double min_sum_hessian, double lambda_l2,
                             int64_t* records, void* stream) {
  if (!ctx || n_hist < 0 || k < 0 || ((int64_t)n_hist * k > 0 && (!hist || !n_bins || !records)) ||
      (int64_t)n_hist * k >= ((int64_t)1 << 24)) {
    set_error("train_split_scan: bad arguments"); return OTTOHIP_EINVAL;
  }
  if (n_hist == 0 || k == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  k_tr_scan<<<(unsigned)(n_hist * k), TR_T, 0, s>>>(reinterpret_cast<const long long*>(hist), k, n_bins,
                                                    std::ldexp(1.0, e_g - 15), std::ldexp(1.0, e_h - 15),
                                                    (long long)min_child_samples, min_sum_hessian, lambda_l2,
                                                    reinterpret_cast<long long*>(records));
  OH_HIP(hipGetLastError());
  return 0;
}

int ottohip_train_partition(ottohip_ctx* ctx, const uint8_t* bins, int stride, int64_t n_total, int feature, int bin,
                            const int32_t* rows, int64_t n, int32_t* rows_out, int64_t* n_left, void* stream) {
  if (!ctx || stride < 1 || feature < 0 || feature >= stride || n_total < 0 || n < 0 || !n_left ||
      (n > 0 && (!bins || !rows || !rows_out || rows == rows_out))) {
    set_error("train_partition: bad arguments (0 <= feature < stride, rows_out another buffer than rows)");
    return OTTOHIP_EINVAL;
  }
  *n_left = 0;
  if (n == 0) return 0;
  if (ceil_div(n, TR_T) >= ((int64_t)1 << 31)) { set_error("train_partition: too many rows"); return OTTOHIP_ELIMIT; }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const int64_t nt = ceil_div(n, TR_T);
  uint32_t* cnt = nullptr;
  uint64_t *toff = nullptr, *total = nullptr;
  int* err = nullptr;
  OH_TRY(ctx->ws.get("tr_pcnt", (size_t)nt, &cnt));
  OH_TRY(ctx->ws.get("tr_poff", (size_t)nt, &toff));
  OH_TRY(ctx->ws.get("tr_ptot", 1, &total));
  OH_TRY(tr_err(ctx, s, &err));
  ctx->reset_timing();
  const int ph = ctx->begin("train_partition", s, (double)n * 10.0);
  k_tr_pcount<<<(unsigned)nt, TR_T, 0, s>>>(bins, stride, n_total, feature, bin, rows, n, cnt, err);
  OH_TRY(exclusive_scan_u32(ctx, cnt, toff, nt, total, s));
  k_tr_pscatter<<<(unsigned)nt, TR_T, 0, s>>>(bins, stride, n_total, feature, bin, rows, n, toff, total, rows_out);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  uint64_t ht = 0;
  OH_TRY(d2h(&ht, total, 1, s));
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) { set_error("train_partition: a row index is outside the binned matrix"); return OTTOHIP_ERANGE; }
  *n_left = (int64_t)ht;
  return 0;
}

int ottohip_train_apply(ottohip_ctx* ctx, const uint8_t* bins, int stride, int64_t n_rows, const int32_t* split_feature,
                        const int32_t* split_bin, const int32_t* left_child, const int32_t* right_child,
                        const double* leaf_value, int n_leaves, double* scores, void* stream) {
  if (!ctx || stride < 1 || n_rows < 0 || n_leaves < 1 || n_leaves > (1 << 16) || !leaf_value ||
      (n_leaves > 1 && (!split_feature || !split_bin || !left_child || !right_child)) ||
      (n_rows > 0 && (!bins || !scores))) {
    set_error("train_apply: bad arguments"); return OTTOHIP_EINVAL;
  }
  if (n_rows == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  int* err = nullptr;
  OH_TRY(tr_err(ctx, s, &err));
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n_rows, TR_T), (int64_t)ctx->n_cu * 16);
  ctx->reset_timing();
  const int ph = ctx->begin("train_apply", s, (double)n_rows * 20.0);
  k_tr_apply<<<grid, TR_T, 0, s>>>(bins, stride, n_rows, split_feature, split_bin, left_child, right_child, leaf_value,
                                   n_leaves, scores, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) { set_error("train_apply: the tree leaves its arrays or reads a feature outside the matrix"); return OTTOHIP_EINVAL; }
  return 0;
}

int ottohip_train_ndcg(ottohip_ctx* ctx, const double* scores, const int8_t* labels, const int64_t* off,
                       int64_t n_sessions, int64_t n_rows, const double* gain, const double* disc,
                       const double* inv_max_dcg, int k, double* out, void* stream) {
  if (!ctx || n_sessions < 0 || n_rows < 0 || k < 1 || k > TR_NDCG_K || !gain || !disc ||
      (n_sessions > 0 && (!off || !inv_max_dcg || !out)) || (n_rows > 0 && (!scores || !labels))) {
    set_error("train_ndcg: bad arguments (1 <= k <= %d)", TR_NDCG_K); return OTTOHIP_EINVAL;
  }
  if (n_sessions == 0) return 0;
  if (ceil_div(n_sessions, TR_WAVES) >= ((int64_t)1 << 31)) { set_error("train_ndcg: too many sessions"); return OTTOHIP_ELIMIT; }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  int* err = nullptr;
  OH_TRY(tr_err(ctx, s, &err));
  ctx->reset_timing();
  const int ph = ctx->begin("train_ndcg", s, (double)n_rows * 9.0);
  k_tr_ndcg<<<(unsigned)ceil_div(n_sessions, TR_WAVES), TR_T, 0, s>>>(scores, labels, off, n_sessions, n_rows, gain, disc,
                                                                      inv_max_dcg, k, out, err);
  ctx->end(ph, s);
  OH_HIP(hipGetLastError());
  int herr = 0;
  OH_TRY(d2h(&herr, err, 1, s));
  if (herr) { set_error("train_ndcg: a label is outside [0, %d]", TR_MAX_LABEL); return OTTOHIP_ERANGE; }
  return 0;
}

int ottohip_trainer_create(ottohip_ctx* ctx, const uint8_t* bins, int stride, int64_t n_rows, const int32_t* n_bins,
                           int n_features, const int8_t* labels, const int64_t* off, int64_t n_sessions,
                           const ottohip_train_tables* tables, const ottohip_train_params* params,
                           ottohip_trainer** out) {
  if (!ctx || !out || !tables || !params || !n_bins || stride < 1 || n_features < 1 || n_features > stride ||
      n_rows < 0 || n_rows >= ((int64_t)1 << 31) || n_sessions < 0 || n_sessions >= ((int64_t)1 << 31) || !off ||
      (n_rows > 0 && (!bins || !labels)) || !tables->gain || !tables->disc || !tables->sig || !tables->log2t ||
      (n_sessions > 0 && !tables->inv_max_dcg) || tables->n_sig < 2 || tables->truncation_level < 1 ||
      !(tables->sigma > 0.0) || params->num_leaves < 2 || params->num_leaves > (1 << 16) ||
      !(params->colsample_bytree > 0.0) || !(params->colsample_bytree <= 1.0) || params->min_child_samples < 0) {
    set_error("trainer_create: bad arguments (n_features <= stride, rows and sessions below 2^31, 2 <= num_leaves <= "
              "65536, 0 < colsample_bytree <= 1, tables as for train_gradients)");
    return OTTOHIP_EINVAL;
  }
  *out = nullptr;
  OH_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> hoff((size_t)n_sessions + 1);
  std::vector<int8_t> hlab((size_t)n_rows);
  OH_TRY(d2h(hoff.data(), off, hoff.size(), nullptr));
  if (n_rows > 0) OH_TRY(d2h(hlab.data(), labels, hlab.size(), nullptr));
  bool big = false;
  for (int64_t s = 0; s < n_sessions; ++s) {
    const int64_t n = hoff[(size_t)s + 1] - hoff[(size_t)s];
    if (n < 0 || hoff[(size_t)s + 1] - hoff[0] > n_rows) {
      set_error("trainer_create: the session offsets do not ascend inside the frame"); return OTTOHIP_EINVAL;
    }
    if (n > TR_MAX_SESSION) {
      set_error("trainer_create: a session has more than %d rows", TR_MAX_SESSION); return OTTOHIP_ELIMIT;
    }
    big = big || n > TR_LDS_ROWS;
  }
  for (int8_t l : hlab)
    if (l < 0 || l > TR_MAX_LABEL) {
      set_error("trainer_create: a label is outside [0, %d]", TR_MAX_LABEL); return OTTOHIP_ERANGE;
    }
  ottohip_trainer* t = new ottohip_trainer();
  t->ctx = ctx; t->bins = bins; t->stride = stride; t->n = n_rows; t->S = n_sessions;
  t->labels = labels; t->off = off; t->T = *tables; t->P = *params; t->big = big;
  for (int f = 0; f < n_features; ++f) {
    t->n_bins.push_back(std::min(std::max(n_bins[f], 0), TR_BINS));
    if (n_bins[f] > 1) t->valid.push_back(f);
  }
  t->k_max = std::max<int>(1, (int)t->valid.size());
  const size_t n = (size_t)n_rows, ni = (size_t)params->num_leaves - 1;
  int rc = 0;
  if ((rc = tr_alloc(&t->scores, n, "scores")) || (rc = tr_alloc(&t->g, n, "g")) || (rc = tr_alloc(&t->h, n, "h")) ||
      (rc = tr_alloc(&t->gh, n, "gh")) || (rc = tr_alloc(&t->rows, n, "rows")) || (rc = tr_alloc(&t->tmp, n, "rows_tmp")) ||
      (rc = tr_alloc(&t->feats, (size_t)t->k_max, "feats")) || (rc = tr_alloc(&t->nb, (size_t)t->k_max, "n_bins")) ||
      (rc = tr_alloc(&t->hist, (size_t)params->num_leaves * t->k_max * TR_BINS * 3, "histograms")) ||
      (rc = tr_alloc(&t->rec, (size_t)2 * t->k_max * TR_REC, "records")) || (rc = tr_alloc(&t->tree, 4 * ni, "tree")) ||
      (rc = tr_alloc(&t->lv, ni + 1, "leaf values")) || (rc = tr_alloc(&t->mx, 2, "max")) ||
      (rc = tr_alloc(&t->info, 4, "info")) || (rc = tr_alloc(&t->err, 1, "err")) ||
      (big && ((rc = tr_alloc(&t->g_ss, n, "sorted scores")) || (rc = tr_alloc(&t->g_sa, n, "lambda sums")) ||
               (rc = tr_alloc(&t->g_si, n, "sorted rows")) || (rc = tr_alloc(&t->g_sl, n, "sorted labels"))))) {
    ottohip_trainer_free(t);
    return rc;
  }
  if (hipMemset(t->scores, 0, std::max<size_t>(n, 1) * sizeof(double)) != hipSuccess) {
    ottohip_trainer_free(t);
    set_error("trainer_create: hipMemset failed"); return OTTOHIP_EHIP;
  }
  *out = t;
  return 0;
}

void ottohip_trainer_free(ottohip_trainer* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  void* bufs[] = {t->scores, t->g, t->h, t->gh, t->rows, t->tmp, t->feats, t->nb, t->hist, t->rec, t->tree, t->lv,
                  t->mx, t->info, t->err, t->g_ss, t->g_sa, t->g_si, t->g_sl};
  for (void* p : bufs)
    if (p) dev_free(p);
  delete t;
}

int ottohip_trainer_boost(ottohip_trainer* t, int* n_leaves, void* stream) {
  if (!t || !n_leaves) { set_error("trainer_boost: bad arguments"); return OTTOHIP_EINVAL; }
  *n_leaves = 0;
  if (t->n == 0 || t->S == 0) return 0;
  OH_HIP(hipSetDevice(t->ctx->device));
  hipStream_t s = S(stream);
  const int64_t n = t->n;
  OH_HIP(hipMemsetAsync(t->err, 0, sizeof(int), s));
  OH_HIP(hipMemsetAsync(t->g, 0, (size_t)n * sizeof(double), s));
  OH_HIP(hipMemsetAsync(t->h, 0, (size_t)n * sizeof(double), s));
  OH_HIP(hipMemsetAsync(t->mx, 0, 2 * sizeof(unsigned long long), s));
  k_tr_grad<<<(unsigned)t->S, TR_T, 0, s>>>(t->scores, t->labels, t->off, t->S, n, t->T, t->g, t->h, 0, nullptr, nullptr,
                                            nullptr, nullptr, t->err);
  if (t->big)
    k_tr_grad<<<(unsigned)t->S, TR_T, 0, s>>>(t->scores, t->labels, t->off, t->S, n, t->T, t->g, t->h, 1, t->g_ss,
                                              t->g_sa, t->g_si, t->g_sl, t->err);
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, TR_T), (int64_t)t->ctx->n_cu * 8);
  k_tr_absmax<<<grid, TR_T, 0, s>>>(t->g, t->h, n, t->mx);
  k_tr_quant<<<grid, TR_T, 0, s>>>(t->g, t->h, n, t->mx, t->gh, t->info);
  OH_HIP(hipGetLastError());
  int hinfo[3] = {0, 0, 0}, herr = 0;
  OH_TRY(d2h(hinfo, t->info, 3, s));  // the reads of this iteration: exponents and flags
  OH_TRY(d2h(&herr, t->err, 1, s));
  if (herr & ~TR_ERR_BIG) {
    set_error("trainer_boost: the gradients report flags %d (a label outside [0, %d] or a NaN score)", herr, TR_MAX_LABEL);
    return OTTOHIP_ERANGE;
  }
  if (hinfo[2]) return 0;  // max |g| == 0: training ends
  OH_HIP(hipMemsetAsync(t->err, 0, sizeof(int), s));
  int nl = 0;
  OH_TRY(tr_grow(t, hinfo[0], hinfo[1], &nl, s));
  if (nl == 0) return 0;
  const size_t ni = (size_t)nl - 1;
  OH_HIP(hipMemcpyAsync(t->tree, t->sf.data(), ni * 4, hipMemcpyHostToDevice, s));
  OH_HIP(hipMemcpyAsync(t->tree + ni, t->sb.data(), ni * 4, hipMemcpyHostToDevice, s));
  OH_HIP(hipMemcpyAsync(t->tree + 2 * ni, t->lc.data(), ni * 4, hipMemcpyHostToDevice, s));
  OH_HIP(hipMemcpyAsync(t->tree + 3 * ni, t->rc.data(), ni * 4, hipMemcpyHostToDevice, s));
  OH_HIP(hipMemcpyAsync(t->lv, t->lval.data(), (size_t)nl * 8, hipMemcpyHostToDevice, s));
  k_tr_apply<<<(unsigned)std::min<int64_t>(ceil_div(n, TR_T), (int64_t)t->ctx->n_cu * 16), TR_T, 0, s>>>(
      t->bins, t->stride, n, t->tree, t->tree + ni, t->tree + 2 * ni, t->tree + 3 * ni, t->lv, nl, t->scores, t->err);
  OH_HIP(hipGetLastError());
  OH_TRY(d2h(&herr, t->err, 1, s));  // partition, histogram and apply flags of the whole tree
  if (herr) { set_error("trainer_boost: an index left the binned matrix (flags %d)", herr); return OTTOHIP_ERANGE; }
  t->n_trees += 1;
  *n_leaves = nl;
  return 0;
}

int ottohip_trainer_tree(const ottohip_trainer* t, int cap_leaves, int32_t* split_feature, int32_t* split_bin,
                         double* split_gain, int32_t* left_child, int32_t* right_child, double* internal_value,
                         double* internal_weight, int64_t* internal_count, double* leaf_value, double* leaf_weight,
                         int64_t* leaf_count, int* n_leaves) {
  if (!t || !n_leaves || t->n_trees == 0 || t->lval.empty()) {
    set_error("trainer_tree: no tree has been boosted"); return OTTOHIP_EINVAL;
  }
  const int nl = (int)t->lval.size(), ni = nl - 1;
  *n_leaves = nl;
  if (cap_leaves < nl || !split_feature || !split_bin || !split_gain || !left_child || !right_child ||
      !internal_value || !internal_weight || !internal_count || !leaf_value || !leaf_weight || !leaf_count) {
    set_error("trainer_tree: the tree has %d leaves, the arrays hold %d (or one is NULL)", nl, cap_leaves);
    return OTTOHIP_EINVAL;
  }
  for (int i = 0; i < ni; ++i) {
    split_feature[i] = t->sf[(size_t)i]; split_bin[i] = t->sb[(size_t)i]; split_gain[i] = t->sgain[(size_t)i];
    left_child[i] = t->lc[(size_t)i]; right_child[i] = t->rc[(size_t)i];
    internal_value[i] = t->ival[(size_t)i]; internal_weight[i] = t->iwt[(size_t)i]; internal_count[i] = t->icnt[(size_t)i];
  }
  for (int i = 0; i < nl; ++i) {
    leaf_value[i] = t->lval[(size_t)i]; leaf_weight[i] = t->lwt[(size_t)i]; leaf_count[i] = t->lcnt[(size_t)i];
  }
  return 0;
}

int ottohip_trainer_scores(const ottohip_trainer* t, double* scores, void* stream) {
  if (!t || (t->n > 0 && !scores)) { set_error("trainer_scores: bad arguments"); return OTTOHIP_EINVAL; }
  if (t->n == 0) return 0;
  OH_HIP(hipSetDevice(t->ctx->device));
  OH_HIP(hipMemcpyAsync(scores, t->scores, (size_t)t->n * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

}  // extern "C"
